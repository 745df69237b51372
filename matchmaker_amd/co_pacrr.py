"""Drop-in CO-PACRR for matchmaker (matchmaker/models/co_pacrr.py): same constructor / from_config / forward surface, attribute
names and state_dict keys (`convolutions.<n-2>.1.{weight,bias}`, `dense*`).  The cosine match matrix, the n-gram
convolutions with their channel max, the k-max poolings at four document views and the context similarities (:90-158) run
as ONE launch in libmm_native.so (mm_co_pacrr_fwd); the dense layers (:168-179) stay torch.  The conv Sequentials and the
`doc_context_pool` / `masked_softmax` modules are kept (neither of the last two has parameters), so reference checkpoints
load with strict=True; the Conv2d parameters are what the kernel reads.  Selected by models/all.py:162-164.

Reference behaviour kept:
  * masks never enter: padded document columns take part in every top-k and context window, padded query rows are scored
    like real ones and count in the query context's mean;
  * the idf softmax (:160) and the query shuffle (:166) feed a tensor that is never used: both are dropped, except that in
    train() mode the one torch.randperm(Q) call of :166 is still made, so the global CPU generator advances as in the
    reference;
  * forward(..., output_secondary_output=True) returns (score, {}) (:180-181);
  * a view narrower than k raises, as torch.topk does in the reference (here: NativeError, a RuntimeError).
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops, torch_ops  # noqa: F401  (torch_ops registers torch.ops.mm_native.co_pacrr_kmax)


class _MaskedSoftmax(nn.Module):
    """matchmaker.modules.masked_softmax.MaskedSoftmax (no parameters), kept as the `masked_softmax` attribute; CO-PACRR's
    forward only feeds it into dead code (co_pacrr.py:160)."""

    def __init__(self):
        super().__init__()
        self.softmax = nn.Softmax(1)

    def forward(self, x, mask=None):
        if mask is not None:
            mask = mask.float()
            x_masked = x * mask + (1 - 1 / mask)
        else:
            x_masked = x
        x_max = x_masked.max(1)[0]
        x_exp = (x - x_max.unsqueeze(-1)).exp()
        if mask is not None:
            x_exp = x_exp * mask
        return x_exp / x_exp.sum(1).unsqueeze(-1)


class CO_PACRR(nn.Module):
    """Co-PACRR: A Context-Aware Neural IR Model for Ad-hoc Retrieval, Hui et al., WSDM'18 — native k-max pooling."""

    @staticmethod
    def from_config(config, word_embeddings_out_dim):            # co_pacrr.py:31-37
        return CO_PACRR(unified_query_length=config["pacrr_unified_query_length"],
                        unified_document_length=config["pacrr_unified_document_length"],
                        max_conv_kernel_size=config["pacrr_max_conv_kernel_size"],
                        conv_output_size=config["pacrr_conv_output_size"],
                        kmax_pooling_size=config["pacrr_kmax_pooling_size"])

    def __init__(self, unified_query_length: int, unified_document_length: int, max_conv_kernel_size: int,
                 conv_output_size: int, kmax_pooling_size: int):
        super().__init__()
        self.unified_query_length = unified_query_length
        self.unified_document_length = unified_document_length
        self.convolutions = nn.ModuleList([                                              # :55-62
            nn.Sequential(nn.ConstantPad2d((0, i - 1, 0, i - 1), 0),
                          nn.Conv2d(kernel_size=i, in_channels=1, out_channels=conv_output_size),
                          nn.MaxPool3d(kernel_size=(conv_output_size, 1, 1)))
            for i in range(2, max_conv_kernel_size + 1)])
        context_pool_size = 6
        self.doc_context_pool = nn.Sequential(nn.ConstantPad1d((0, context_pool_size - 1), 0),   # :63-66
                                              nn.AvgPool1d(kernel_size=context_pool_size, stride=1))
        self.masked_softmax = _MaskedSoftmax()
        self.kmax_pooling_size = kmax_pooling_size
        self.kmax_pooling_views = ops.co_pacrr_views(unified_document_length)          # :73-74
        self.dense = nn.Linear(len(self.kmax_pooling_views) * 2 * kmax_pooling_size * unified_query_length
                               * max_conv_kernel_size, out_features=100, bias=True)
        self.dense2 = nn.Linear(100, out_features=10, bias=True)
        self.dense3 = nn.Linear(10, out_features=1, bias=False)                        # :76-78

    def _conv_params(self):
        return [c[1].weight for c in self.convolutions], [c[1].bias for c in self.convolutions]

    def per_query_results(self, query_embeddings: torch.Tensor, document_embeddings: torch.Tensor,
                          pairs_per_query: int = 1) -> torch.Tensor:
        """[B, Q, 8 k N] of :158 (per path 0, 2, .., N: the 4k view values, then their 4k contexts).  With gradients
        enabled it goes through torch.ops.mm_native.co_pacrr_kmax (native forward + backward); otherwise one forward launch
        that saves nothing."""
        ws, bs = self._conv_params()
        q, d = query_embeddings.float(), document_embeddings.float()
        k, views = self.kmax_pooling_size, self.kmax_pooling_views
        needs_grad = torch.is_grad_enabled() and (q.requires_grad or d.requires_grad or any(w.requires_grad for w in ws)
                                                  or any(b.requires_grad for b in bs))
        if needs_grad:
            return torch.ops.mm_native.co_pacrr_kmax(q, d, ws, bs, k, views, pairs_per_query)[0]
        return ops.co_pacrr_kmax(q, d, ws, bs, k, views, pairs_per_query=pairs_per_query)

    def forward(self, query_embeddings: torch.Tensor, document_embeddings: torch.Tensor,
                query_pad_oov_mask: torch.Tensor, document_pad_oov_mask: torch.Tensor,
                query_idfs: torch.Tensor, document_idfs: torch.Tensor,
                output_secondary_output: bool = False) -> torch.Tensor:
        """co_pacrr.py:80-181 — same arguments; masks and idfs do not enter (as in the reference)."""
        per_query_results = self.per_query_results(query_embeddings, document_embeddings)
        if self.training:
            torch.randperm(per_query_results.shape[1])        # :166's draw (its result is unused there too)
        all_flat = per_query_results.view(per_query_results.shape[0], -1)              # :168
        dense_out = F.relu(self.dense(all_flat))
        dense_out = F.relu(self.dense2(dense_out))
        dense_out = self.dense3(dense_out)
        output = torch.squeeze(dense_out, 1)                                             # :179
        if output_secondary_output:
            return output, {}
        return output

    def get_param_stats(self):                                                           # :184-185
        return "CO-PACRR: / "

    def get_param_secondary(self):                                                       # :187-188
        return {}
