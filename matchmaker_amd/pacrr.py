"""Drop-in PACRR for matchmaker (matchmaker/models/pacrr.py): same constructor / from_config / forward surface and
state_dict keys (`convolutions.<n-2>.1.{weight,bias}`, `dense*`).  The cosine match matrix, the n-gram convolutions with
their channel max and the three k-max poolings (:78-97) run as ONE launch in libmm_native.so (mm_pacrr_fwd); the dense
layers (:101-112) stay torch.  The nn.Sequential(ConstantPad2d, Conv2d, MaxPool3d) modules are kept, so reference
checkpoints load with strict=True; their Conv2d parameters are what the kernel reads.  Selected by models/all.py:159-161.

Reference behaviour kept:
  * masks never enter: padded document columns take part in every top-k, padded query rows are scored like real ones;
  * the idf softmax of :99 is dead code there (:101 flattens the unweighted tensor): query_idfs / document_idfs are ignored;
  * forward returns the score tensor only, also with output_secondary_output=True (:113);
  * D < k raises, as torch.topk does in the reference (here: NativeError, a RuntimeError).
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops, torch_ops  # noqa: F401  (torch_ops registers torch.ops.mm_native.pacrr_kmax)


class PACRR(nn.Module):
    """PACRR: A Position-Aware Neural IR Model for Relevance Matching, Hui et al., EMNLP'17 — native k-max pooling."""

    @staticmethod
    def from_config(config, word_embeddings_out_dim):            # pacrr.py:26-32
        return PACRR(unified_query_length=config["pacrr_unified_query_length"],
                     unified_document_length=config["pacrr_unified_document_length"],
                     max_conv_kernel_size=config["pacrr_max_conv_kernel_size"],
                     conv_output_size=config["pacrr_conv_output_size"],
                     kmax_pooling_size=config["pacrr_kmax_pooling_size"])

    def __init__(self, unified_query_length: int, unified_document_length: int, max_conv_kernel_size: int,
                 conv_output_size: int, kmax_pooling_size: int):
        super().__init__()
        self.unified_query_length = unified_query_length
        self.unified_document_length = unified_document_length
        self.convolutions = nn.ModuleList([                                              # :53-59
            nn.Sequential(nn.ConstantPad2d((0, i - 1, 0, i - 1), 0),
                          nn.Conv2d(kernel_size=i, in_channels=1, out_channels=conv_output_size),
                          nn.MaxPool3d(kernel_size=(conv_output_size, 1, 1)))
            for i in range(2, max_conv_kernel_size + 1)])
        self.kmax_pooling_size = kmax_pooling_size
        self.dense = nn.Linear(kmax_pooling_size * unified_query_length * max_conv_kernel_size, out_features=100, bias=True)
        self.dense2 = nn.Linear(100, out_features=10, bias=True)
        self.dense3 = nn.Linear(10, out_features=1, bias=False)                        # :64-66

    def _conv_params(self):
        return [c[1].weight for c in self.convolutions], [c[1].bias for c in self.convolutions]

    def per_query_results(self, query_embeddings: torch.Tensor, document_embeddings: torch.Tensor,
                          pairs_per_query: int = 1) -> torch.Tensor:
        """[B, Q, k N] of :97 (paths 0, 2, .., N).  With gradients enabled it goes through torch.ops.mm_native.pacrr_kmax
        (native forward + backward); otherwise one forward launch that saves nothing."""
        ws, bs = self._conv_params()
        q, d = query_embeddings.float(), document_embeddings.float()
        needs_grad = torch.is_grad_enabled() and (q.requires_grad or d.requires_grad or any(w.requires_grad for w in ws)
                                                  or any(b.requires_grad for b in bs))
        if needs_grad:
            return torch.ops.mm_native.pacrr_kmax(q, d, ws, bs, self.kmax_pooling_size, pairs_per_query)[0]
        return ops.pacrr_kmax(q, d, ws, bs, self.kmax_pooling_size, pairs_per_query=pairs_per_query)

    def forward(self, query_embeddings: torch.Tensor, document_embeddings: torch.Tensor,
                query_pad_oov_mask: torch.Tensor, document_pad_oov_mask: torch.Tensor,
                query_idfs: torch.Tensor, document_idfs: torch.Tensor,
                output_secondary_output: bool = False) -> torch.Tensor:
        """pacrr.py:68-113 — same arguments; masks and idfs do not enter (as in the reference), only the score is returned."""
        per_query_results = self.per_query_results(query_embeddings, document_embeddings)
        all_flat = per_query_results.view(per_query_results.shape[0], -1)              # :101
        dense_out = F.relu(self.dense(all_flat))
        dense_out = F.relu(self.dense2(dense_out))
        dense_out = self.dense3(dense_out)
        return torch.squeeze(dense_out, 1)                                               # :112-113

    def get_param_stats(self):                                                           # :115-116
        return "PACRR: / "
