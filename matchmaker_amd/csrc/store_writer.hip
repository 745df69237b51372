// Device-side ColBERT store writer for MI355X (gfx950 / CDNA4): a batch of encoder output [n_docs, D, E] -> its non-zero
// token rows appended to a resident token store, with the documents' row ranges (include/mm_native.h).
//
// A stream compaction in three launches on one stream, chained through device memory only:
//   * store_count_kernel   — one workgroup per 64 consecutive rows of the batch (a word; rows are numbered b * D + j, across
//     documents), one wavefront per 16 of them: a 16-lane group per row ORs the magnitude bits of its 16-byte units, a
//     ballot turns the four groups of a step into four row flags, four steps make a quarter of the 64-bit word bits[w].
//     Reads x once, coalesced.
//   * store_scan_kernel    — one workgroup: the exclusive prefix of popcount(bits[w]) over the words, the capacity test
//     against the device-side fill, the new fill and the sticky status.  It leaves the batch's first row (or -1 = refused)
//     in the workspace for the third launch.
//   * store_scatter_kernel — one workgroup per word again, a wavefront per quarter: row i of word w goes to
//     base + pre[w] + popcount(bits[w] below i), a 16-lane group copies / converts it with 16-byte loads and stores and, for
//     an fp8 store, quantises it with the code mm_fp8_quantize_rows runs (fp8_device.h).  Thread b < n_docs writes document
//     b's range from the same prefix.
// Positions come from the scan, never from an atomic: the row order is fixed and two runs give the same bits.  No
// workgroup waits on another inside a launch; the launches are the only synchronisation.
#include "mm_internal.h"
#include "elem_device.h"
#include "fp8_device.h"
#include "scan_select_device.h"

namespace mm {

struct StoreArgs {
  const void* x;
  int64_t n_rows;       // n_docs * D
  int n_docs, D, E;
  int keep_all;         // MM_STORE_KEEP_ZERO_ROWS
  void* rows_out;
  int out_dtype;
  uint8_t* codes;
  float* scales;
  int64_t capacity;
  int64_t* fill;
  int64_t* doc_begin;
  int64_t* doc_end;
  int32_t* status;
  uint64_t* bits;       // [nw] one flag per row
  int32_t* pre;         // [nw + 1] kept rows before word w; pre[nw] = the batch's kept rows
  int64_t* ctrl;        // [0] the store row of the batch's first kept row, -1 = the batch was refused
  int nw;               // ceil(n_rows / 64)
};

static void store_carve(WsCursor& ws, int64_t n_rows, StoreArgs* a) {
  const size_t nw = (size_t)((n_rows + 63) / 64);
  uint64_t* bits = ws.take<uint64_t>(nw);
  int32_t* pre = ws.take<int32_t>(nw + 1);
  int64_t* ctrl = ws.take<int64_t>(1);
  if (a) {
    a->bits = bits; a->pre = pre; a->ctrl = ctrl; a->nw = (int)nw;
  }
}

template <int DT>
__global__ void __launch_bounds__(256) store_count_kernel(const StoreArgs a) {
  // one workgroup per word, one wavefront per quarter of it: wavefront q flags rows 16 q .. 16 q + 15 of the word and writes
  // bits 16 q .. 16 q + 15 of bits[w] (little-endian: the 16-bit store at index 4 w + q)
  const int lane = threadIdx.x & 63, l = lane & 15, g = lane >> 4, q = threadIdx.x >> 6;
  const int w = blockIdx.x;
  const int64_t r0 = (int64_t)w * 64 + 16 * q;
  const int64_t rem = a.n_rows - r0;                  // may be <= 0 in the last word: an empty quarter
  uint32_t m = 0;
  if (a.keep_all) {
    m = rem >= 16 ? 0xffffu : (rem > 0 ? (1u << rem) - 1u : 0u);
  } else if (rem > 0) {
    constexpr int ES = DT == MM_F32 ? 4 : 2;
    constexpr uint32_t kMag = DT == MM_F32 ? 0x7fffffffu : 0x7fff7fffu;   // everything but the sign bits: -0.0 is zero
    const int64_t rowbytes = (int64_t)a.E * ES;
    const int U = (int)(rowbytes >> 4);
    uint32_t nz[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {                     // the loads of the four steps in flight before the first ballot
      const int64_t r = r0 + 4 * k + g;
      nz[k] = 0;
      if (r < a.n_rows) {
        const char* xr = (const char*)a.x + r * rowbytes;
        for (int u = l; u < U; u += 16) {
          const u32x4 v = *(const u32x4*)(xr + u * 16);
          nz[k] |= (v[0] | v[1] | v[2] | v[3]) & kMag;
        }
      }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const uint64_t b = __ballot(nz[k] != 0);
#pragma unroll
      for (int gg = 0; gg < 4; ++gg)
        if ((b >> (16 * gg)) & 0xffffull) m |= 1u << (4 * k + gg);
    }
  }
  if (lane == 0) ((uint16_t*)a.bits)[4 * (int64_t)w + q] = (uint16_t)m;
}

__global__ void __launch_bounds__(1024) store_scan_kernel(const StoreArgs a) {
  __shared__ int32_t part[1024];
  const int t = threadIdx.x;
  const int per = (a.nw + 1023) / 1024;
  const int w0 = t * per < a.nw ? t * per : a.nw;     // (nw <= 2^25 and per <= 2^15: no overflow)
  const int w1 = w0 + per < a.nw ? w0 + per : a.nw;
  int32_t s = 0;
  for (int w = w0; w < w1; ++w) s += __popcll(a.bits[w]);
  part[t] = s;
  block_incl_scan_lds(part, t);
  int32_t run = part[t] - s;
  for (int w = w0; w < w1; ++w) {
    a.pre[w] = run;
    run += __popcll(a.bits[w]);
  }
  if (t == 1023) {
    const int64_t total = part[1023];
    a.pre[a.nw] = (int32_t)total;
    const int32_t st = a.status[0];
    const int64_t f = a.fill[0];
    const bool ok = st == 0 && f >= 0 && f <= a.capacity && total <= a.capacity - f;
    if (ok) {
      a.fill[0] = f + total;
      a.ctrl[0] = f;
    } else {
      a.ctrl[0] = -1;
      if (st == 0) a.status[0] = 1;
    }
  }
}

// kept rows of the batch before row r (0 <= r <= n_rows)
__device__ __forceinline__ int64_t kept_before(const StoreArgs& a, int64_t r) {
  const int w = (int)(r >> 6), i = (int)(r & 63);
  int64_t n = a.pre[w];
  if (i) n += __popcll(a.bits[w] & ((1ull << i) - 1ull));   // (i != 0 means r < 64 nw: the word exists)
  return n;
}

template <int ODT>
__device__ __forceinline__ uint32_t pack2(float lo, float hi) {
  if constexpr (ODT == MM_F16) {
    f16x2_t h;
    h[0] = (_Float16)lo;                                     // v_cvt_f16_f32: nearest even, overflow to inf, fp16 subnormals kept
    h[1] = (_Float16)hi;
    return __builtin_bit_cast(uint32_t, h);
  } else {
    return bf16_rne_bits(lo) | (bf16_rne_bits(hi) << 16);      // finite input (elem_device.h)
  }
}

// One 16-lane group copies the row at xr [E] of type DT to orow [E] of type odt (lane l of the group).
template <int DT>
__device__ __forceinline__ void store_row(const char* xr, char* orow, int E, int odt, int l) {
  constexpr int ES = DT == MM_F32 ? 4 : 2;
  if (odt == DT) {                                           // the bits, 16 bytes at a time
    const int U = (E * ES) >> 4;
    for (int u = l; u < U; u += 16) *(u32x4*)(orow + u * 16) = *(const u32x4*)(xr + u * 16);
  } else if constexpr (DT != MM_F32) {                       // 16-bit -> fp32, exact (E % 8 == 0: the rows are 16-byte multiples)
    const int nu = E >> 3;
    for (int u = l; u < nu; u += 16) {
      float v[8];
      load8<DT>(xr, u, v);
      *(f32x4*)(orow + u * 32) = f32x4{v[0], v[1], v[2], v[3]};
      *(f32x4*)(orow + u * 32 + 16) = f32x4{v[4], v[5], v[6], v[7]};
    }
  } else if (E & 7) {                                        // fp32 -> fp16 / bf16 at E % 8 == 4: the output rows are 8-byte
    const int n4 = E >> 2;                                   // multiples only, so 16-byte loads and 8-byte stores
    for (int u = l; u < n4; u += 16) {
      const f32x4 v = *(const f32x4*)(xr + u * 16);
      u32x2 o;
      o[0] = odt == MM_F16 ? pack2<MM_F16>(v[0], v[1]) : pack2<MM_BF16>(v[0], v[1]);
      o[1] = odt == MM_F16 ? pack2<MM_F16>(v[2], v[3]) : pack2<MM_BF16>(v[2], v[3]);
      *(u32x2*)(orow + u * 8) = o;
    }
  } else {                                                   // fp32 -> fp16 / bf16
    const int nu = E >> 3;
    for (int u = l; u < nu; u += 16) {
      float v[8];
      load8<MM_F32>(xr, u, v);
      u32x4 o;
#pragma unroll
      for (int j = 0; j < 4; ++j) o[j] = odt == MM_F16 ? pack2<MM_F16>(v[2 * j], v[2 * j + 1]) : pack2<MM_BF16>(v[2 * j], v[2 * j + 1]);
      *(u32x4*)(orow + u * 16) = o;
    }
  }
}

template <int DT>
__global__ void __launch_bounds__(256) store_scatter_kernel(const StoreArgs a) {
  const int64_t base = a.ctrl[0];
  if (base < 0) return;                                      // refused (or a sticky status): nothing is written
  const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (gid < a.n_docs) {                                      // the grid has 256 nw >= n_rows >= n_docs threads
    const int64_t r = gid * a.D;
    a.doc_begin[gid] = base + kept_before(a, r);
    a.doc_end[gid] = base + kept_before(a, r + a.D);
  }
  const int lane = threadIdx.x & 63, l = lane & 15, g = lane >> 4, q = threadIdx.x >> 6;
  const int w = blockIdx.x;                                  // one workgroup per word, wavefront q its rows 16 q .. 16 q + 15
  const uint64_t m = a.bits[w];
  if (((m >> (16 * q)) & 0xffffull) == 0) return;            // nothing kept in this quarter
  constexpr int ES = DT == MM_F32 ? 4 : 2;
  const int64_t pos0 = base + a.pre[w];
  const int OS = a.out_dtype == MM_F32 ? 4 : 2;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int i = 16 * q + 4 * k + g;
    if (!((m >> i) & 1ull)) continue;                        // (a whole 16-lane group skips)
    const int64_t dst = pos0 + __popcll(m & ((1ull << i) - 1ull));   // < base + total <= capacity (store_scan_kernel)
    const char* xr = (const char*)a.x + ((int64_t)w * 64 + i) * a.E * ES;
    if (a.rows_out) store_row<DT>(xr, (char*)a.rows_out + dst * a.E * OS, a.E, a.out_dtype, l);
    if (a.codes) fp8_quantize_row<DT>(xr, a.E, l, a.codes + dst * a.E, a.scales + dst);
  }
}

template <int DT>
static int launch_store(const StoreArgs& a, hipStream_t stream) {
  const dim3 grid((unsigned)a.nw), block(256);
  hipLaunchKernelGGL(store_count_kernel<DT>, grid, block, 0, stream, a);
  if (int e = check_launch("store_count_kernel")) return e;
  hipLaunchKernelGGL(store_scan_kernel, dim3(1), dim3(1024), 0, stream, a);
  if (int e = check_launch("store_scan_kernel")) return e;
  hipLaunchKernelGGL(store_scatter_kernel<DT>, grid, block, 0, stream, a);
  return check_launch("store_scatter_kernel");
}

}  // namespace mm

using namespace mm;

extern "C" size_t mm_store_append_workspace_bytes(int n_docs, int D) {
  if (n_docs <= 0 || D <= 0) return 0;
  WsCursor ws;
  store_carve(ws, (int64_t)n_docs * D, nullptr);
  return ws.used;
}

extern "C" int mm_store_append(const void* x, int n_docs, int D, int E, int dtype, int flags, void* rows_out, int out_dtype,
                               uint8_t* codes_out, float* scales_out, int64_t capacity, int64_t* fill, int64_t* doc_begin,
                               int64_t* doc_end, int32_t* status, void* workspace, size_t workspace_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (n_docs < 0 || D <= 0 || E <= 0 || capacity < 0) return set_error(MM_EINVAL, "store_append: bad shape");
  if (dtype != MM_F32 && dtype != MM_F16 && dtype != MM_BF16) return set_error(MM_EINVAL, "store_append: bad dtype %d", dtype);
  if (flags & ~MM_STORE_KEEP_ZERO_ROWS) return set_error(MM_EINVAL, "store_append: unknown flags 0x%x", flags);
  if (!rows_out && !codes_out && !scales_out) return set_error(MM_EINVAL, "store_append: neither rows_out nor codes_out / scales_out given");
  if (!codes_out != !scales_out) return set_error(MM_EINVAL, "store_append: codes_out and scales_out go together");
  if (rows_out) {
    if (out_dtype != MM_F32 && out_dtype != MM_F16 && out_dtype != MM_BF16)
      return set_error(MM_EINVAL, "store_append: bad out_dtype %d", out_dtype);
    if (out_dtype != dtype && out_dtype != MM_F32 && dtype != MM_F32)
      return set_error(MM_EUNSUPPORTED, "store_append: fp16 <-> bf16 is not a conversion the store makes (convert the batch)");
  }
  const int es = dtype == MM_F32 ? 4 : 2;
  if (((int64_t)E * es) % 16)
    return set_error(MM_EUNSUPPORTED, "store_append: a row of E=%d elements of %d bytes is not a multiple of 16 bytes", E, es);
  if (codes_out && E % 16) return set_error(MM_EUNSUPPORTED, "store_append: an fp8 store needs E %% 16 == 0, got E=%d", E);
  const int64_t n_rows = (int64_t)n_docs * D;
  if (n_rows >= (1LL << 31))
    return set_error(MM_EUNSUPPORTED, "store_append: n_docs * D = %lld rows in one batch, the limit is 2^31 - 1", (long long)n_rows);
  if (n_docs == 0) return MM_OK;
  if (!x || !fill || !doc_begin || !doc_end || !status) return set_error(MM_EINVAL, "store_append: null pointer");
  if ((((uintptr_t)x | (uintptr_t)rows_out | (uintptr_t)codes_out) & 15) || ((uintptr_t)scales_out & 3) ||
      (((uintptr_t)fill | (uintptr_t)doc_begin | (uintptr_t)doc_end) & 7) || ((uintptr_t)status & 3))
    return set_error(MM_EINVAL, "store_append: x / rows_out / codes_out must be 16-byte aligned, fill / doc_begin / doc_end 8, "
                                "scales_out / status 4");
  const size_t need = mm_store_append_workspace_bytes(n_docs, D);
  if (!workspace || workspace_bytes < need) return set_error(MM_EWORKSPACE, "store_append: workspace needs %zu bytes", need);

  StoreArgs a{};
  a.x = x; a.n_rows = n_rows; a.n_docs = n_docs; a.D = D; a.E = E; a.keep_all = (flags & MM_STORE_KEEP_ZERO_ROWS) ? 1 : 0;
  a.rows_out = rows_out; a.out_dtype = rows_out ? out_dtype : dtype; a.codes = codes_out; a.scales = scales_out;
  a.capacity = capacity; a.fill = fill; a.doc_begin = doc_begin; a.doc_end = doc_end; a.status = status;
  WsCursor ws(workspace, workspace_bytes);
  store_carve(ws, n_rows, &a);
  return with_dtype(dtype, [&](auto dt) { return launch_store<MM_V(dt)>(a, stream); });
}
