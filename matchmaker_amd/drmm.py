"""Drop-in DRMM for matchmaker (matchmaker/models/drmm.py): same constructor `DRMM(word_embeddings, bin_count)`, the same
`forward(query, document)` on token dictionaries (both token layouts, :44-53), return shape [B, 1], get_param_stats and the
reference's state_dict keys — allennlp 2.5.1's FeedForward keys `matching_classifier._linear_layers.{0,1}.{weight,bias}`,
`query_gate._linear_layers.{0,1}.{weight,bias}`, plus the embedder's own.  Selected by models/all.py:154.

The reference computes the cosine matrix on the GPU, copies it to the host, calls torch.histc once per (pair, query token)
and copies the histograms back (:66-76).  Here the cosine and the histograms are ONE launch in libmm_native.so
(mm_drmm_fwd) and nothing leaves the device.  eval() without gradients also fuses log1p + matching_classifier + the gated
sum into that launch (ops.drmm_score); otherwise the histogram comes from torch.ops.mm_native.drmm_hist and the head runs
in torch, so autograd trains both FeedForwards (the histogram itself has no gradient: "only works with fixed word
embeddings", :20).

allennlp is not a dependency: FeedForward / Activation.by_name('tanh') are restated from the published 2.x source
(Linear -> activation -> Dropout(0) per layer).  Reference behaviour kept: no mask enters the histogram
(padded document positions count in the bin of cosine 0, padded query rows put all D counts there), a cosine that rounds
above 1 is dropped as histc drops it, and the masked softmax gives NaN for a query whose every token is masked."""
from typing import Dict, List

import torch
import torch.nn as nn

from . import ops, torch_ops  # noqa: F401  (torch_ops registers torch.ops.mm_native.drmm_hist / drmm_score)


class FeedForward(nn.Module):
    """allennlp.modules.feedforward.FeedForward (2.x), restated: per layer Linear -> activation -> Dropout."""

    def __init__(self, input_dim: int, num_layers: int, hidden_dims: List[int], activations: List[nn.Module],
                 dropout: float = 0.0):
        super().__init__()
        assert len(hidden_dims) == num_layers and len(activations) == num_layers
        self._activations = nn.ModuleList(activations)
        input_dims = [input_dim] + hidden_dims[:-1]
        self._linear_layers = nn.ModuleList([nn.Linear(i, o) for i, o in zip(input_dims, hidden_dims)])
        self._dropout = nn.ModuleList([nn.Dropout(p=dropout) for _ in hidden_dims])
        self._output_dim = hidden_dims[-1]
        self.input_dim = input_dim

    def get_output_dim(self):
        return self._output_dim

    def get_input_dim(self):
        return self.input_dim

    def forward(self, inputs: torch.Tensor) -> torch.Tensor:
        output = inputs
        for layer, activation, dropout in zip(self._linear_layers, self._activations, self._dropout):
            output = dropout(activation(layer(output)))
        return output


class MaskedSoftmax(nn.Module):
    """drmm.py:97-120: 1 - 1 / mask is -inf on masked items (NaN for a row with every item masked: kept)."""

    def forward(self, x, mask=None):
        if mask is not None:
            mask = mask.float()
            x_masked = x * mask + (1 - 1 / mask)
        else:
            x_masked = x
        x_max = x_masked.max(1)[0]
        x_exp = (x - x_max.unsqueeze(-1)).exp()
        if mask is not None:
            x_exp = x_exp * mask.float()
        return x_exp / x_exp.sum(1).unsqueeze(-1)


class DRMM(nn.Module):
    """A Deep Relevance Matching Model for Ad-hoc Retrieval, Guo et al., CIKM'16 — native cosine + matching histogram."""

    def __init__(self, word_embeddings: nn.Module, bin_count: int):
        super().__init__()
        self.word_embeddings = word_embeddings
        self.bin_count = bin_count
        E = self.word_embeddings.get_output_dim()
        self.matching_classifier = FeedForward(input_dim=bin_count, num_layers=2, hidden_dims=[bin_count, 1],
                                               activations=[nn.Tanh(), nn.Tanh()])
        self.query_gate = FeedForward(input_dim=E, num_layers=2, hidden_dims=[E, 1], activations=[nn.Tanh(), nn.Tanh()])
        self.query_softmax = MaskedSoftmax()

    def forward(self, query: Dict[str, torch.Tensor], document: Dict[str, torch.Tensor]) -> torch.Tensor:
        if len(query["tokens"].shape) == 2:                                               # :44-53
            query_pad_oov_mask = (query["tokens"] > 1).float()
            document_pad_oov_mask = (document["tokens"] > 1).float()
        else:
            query_pad_oov_mask = (torch.sum(query["tokens"], 2) > 0).float()
            document_pad_oov_mask = (torch.sum(document["tokens"], 2) > 0).float()
        query_embeddings = self.word_embeddings(query) * query_pad_oov_mask.unsqueeze(-1)
        document_embeddings = self.word_embeddings(document) * document_pad_oov_mask.unsqueeze(-1)
        return self.score_embeddings(query_embeddings, document_embeddings, query_pad_oov_mask, document_pad_oov_mask)

    def score_embeddings(self, query_embeddings: torch.Tensor, document_embeddings: torch.Tensor,
                         query_pad_oov_mask: torch.Tensor, document_pad_oov_mask: torch.Tensor = None,
                         pairs_per_query: int = 1) -> torch.Tensor:
        """drmm.py:66-91 on masked embeddings: [B, 1].  pairs_per_query > 1: one query row per group of candidates.
        document_pad_oov_mask (optional): rows past a document's last unmasked position are zero rows, which the kernel
        counts without reading them (the length is computed on the device: no synchronisation)."""
        q, d = query_embeddings.float(), document_embeddings.float()
        d_len = None
        if document_pad_oov_mask is not None:
            pos = torch.arange(1, d.shape[1] + 1, device=d.device, dtype=torch.float32)
            d_len = (document_pad_oov_mask.float() * pos).amax(dim=1).to(torch.int32)
        query_gates_raw = self.query_gate(query_embeddings)                                # :82-83
        query_gates = self.query_softmax(query_gates_raw.squeeze(-1), query_pad_oov_mask)
        lin0, lin1 = self.matching_classifier._linear_layers
        if not self.training and not torch.is_grad_enabled():
            s = ops.drmm_score(q, d, query_gates, lin0.weight, lin0.bias, lin1.weight, lin1.bias,
                               pairs_per_query=pairs_per_query, d_len=d_len)
            return s.unsqueeze(-1)
        hist = torch.ops.mm_native.drmm_hist(q.detach(), d.detach(), self.bin_count, pairs_per_query, d_len)
        classified = self.matching_classifier(torch.log1p(hist))                           # :77
        if pairs_per_query > 1:
            query_gates = query_gates.repeat_interleave(pairs_per_query, dim=0)[:d.shape[0]]
        return torch.sum(classified * query_gates.unsqueeze(-1), dim=1)                    # :88

    def get_param_stats(self):
        return "DRMM: -"
