"""Drop-in MatchPyramid for matchmaker (matchmaker/models/matchpyramid.py): the same from_config / constructor (length check
included), the same `forward(query_embeddings, document_embeddings, query_pad_oov_mask, document_pad_oov_mask,
output_secondary_output)` returning [B] (or `(output, {})`), get_param_stats / get_param_secondary, and the reference's
state_dict keys — `conv_layers.conv <i>.{weight,bias}` (the Sequential is built over the same OrderedDict names "pad i",
"conv i", "relu i", "pool i"), `dense*` — so its checkpoints load with strict=True.  Selected by models/all.py:153.

The reference launches a cosine and, per layer, a pad, a Conv2d, a ReLU and an AdaptiveMaxPool2d, every activation through
HBM.  Here :74-92 is ONE launch in libmm_native.so (mm_matchpyramid_fwd) when the inputs are on the GPU and neither an input
nor a parameter needs a gradient; the three dense layers stay torch.  Otherwise — training (by default), CPU tensors, shapes
the kernel refuses with MM_EUNSUPPORTED — the module's own torch layers run, which are the reference's.  Any other native
error is re-raised.  Training can go through the native pair mm_matchpyramid_fwd_save / mm_matchpyramid_bwd instead: set the
attribute `native_backward = True` (class docstring: why it is off by default).

Reference behaviour kept: the masks never enter; the pad / kernel transposition of :50-51 (pad right by
k[0] - 1 and below by k[1] - 1 for a k[0] x k[1] kernel); allennlp's cosine restated (x / (|x| + 1e-13))."""
from collections import OrderedDict
from typing import List, Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib, ops, torch_ops  # noqa: F401  (torch_ops registers torch.ops.mm_native.matchpyramid_features)


class CosineMatrixAttention(nn.Module):
    """allennlp.modules.matrix_attention.cosine_matrix_attention (2.x), restated: fp32 / fp64 only, as the configs use it."""

    def forward(self, matrix_1: torch.Tensor, matrix_2: torch.Tensor) -> torch.Tensor:
        a_norm = matrix_1 / (matrix_1.norm(p=2, dim=-1, keepdim=True) + 1e-13)
        b_norm = matrix_2 / (matrix_2.norm(p=2, dim=-1, keepdim=True) + 1e-13)
        return torch.bmm(a_norm, b_norm.transpose(-1, -2))


class MatchPyramid(nn.Module):
    """Text Matching as Image Recognition, Pang et al., AAAI'16 — native cosine + conv pyramid + adaptive max pooling.

    native_backward (an attribute, no constructor argument: the reference's signature is kept): when something needs a
    gradient, the inputs are on the GPU and the shape is supported, `features` goes through
    torch.ops.mm_native.matchpyramid_features_train (mm_matchpyramid_fwd_save + mm_matchpyramid_bwd, exact fp32, no atomics)
    instead of the module's torch layers.

    Default False, by measurement (tools/bench_matchpyramid.py on one MI355X, Q30 / D200 / E300, the default pyramid, 64
    pairs, forward + backward of the whole module, both paths in one process): native 2.93 ms, eager 1.33 ms — the native
    step is SLOWER (0.45 x; 2,048 pairs: 33.0 ms against 19.0 ms), so it is opt-in.  DESIGN.md §3.11."""

    native_backward = False

    @staticmethod
    def from_config(config, word_embeddings_out_dim):
        return MatchPyramid(conv_output_size=config["match_pyramid_conv_output_size"],
                            conv_kernel_size=config["match_pyramid_conv_kernel_size"],
                            adaptive_pooling_size=config["match_pyramid_adaptive_pooling_size"])

    def __init__(self, conv_output_size: List[int], conv_kernel_size: List[Tuple[int, int]],
                 adaptive_pooling_size: List[Tuple[int, int]]):
        super().__init__()
        self.cosine_module = CosineMatrixAttention()
        if len(conv_output_size) != len(conv_kernel_size) or len(conv_output_size) != len(adaptive_pooling_size):
            raise Exception("conv_output_size, conv_kernel_size, adaptive_pooling_size must have the same length")
        layers = OrderedDict()
        last = 1
        for i, (c, k, p) in enumerate(zip(conv_output_size, conv_kernel_size, adaptive_pooling_size)):
            layers["pad " + str(i)] = nn.ConstantPad2d((0, k[0] - 1, 0, k[1] - 1), 0)      # :50, transposition kept
            layers["conv " + str(i)] = nn.Conv2d(kernel_size=tuple(k), in_channels=last, out_channels=c)
            layers["relu " + str(i)] = nn.ReLU()
            layers["pool " + str(i)] = nn.AdaptiveMaxPool2d(tuple(p))
            last = c
        self.conv_layers = nn.Sequential(layers)
        self.pool_sizes = [(int(p[0]), int(p[1])) for p in adaptive_pooling_size]
        self.dense = nn.Linear(conv_output_size[-1] * adaptive_pooling_size[-1][0] * adaptive_pooling_size[-1][1],
                               out_features=100, bias=True)
        self.dense2 = nn.Linear(100, out_features=10, bias=True)
        self.dense3 = nn.Linear(10, out_features=1, bias=False)
        self._packed = None      # (key, packed weights, packed biases): the kernel's parameter layout, rebuilt when a conv changes

    def _convs(self):
        return [m for m in self.conv_layers if isinstance(m, nn.Conv2d)]

    def _packed_params(self, convs):
        key = tuple((c.weight.data_ptr(), c.weight._version, c.bias.data_ptr(), c.bias._version) for c in convs)
        if self._packed is None or self._packed[0] != key:
            w, b = ops.matchpyramid_pack([c.weight for c in convs], [c.bias for c in convs])
            self._packed = (key, w, b)
        return self._packed[1], self._packed[2]

    def torch_features(self, query_embeddings: torch.Tensor, document_embeddings: torch.Tensor) -> torch.Tensor:
        """:74-92 in torch ops (the reference's own layers): the training / CPU / out-of-envelope path."""
        cosine_matrix = self.cosine_module.forward(query_embeddings, document_embeddings)[:, None, :, :]
        conv_result = self.conv_layers(cosine_matrix)
        return conv_result.view(conv_result.size(0), -1)

    def features(self, query_embeddings: torch.Tensor, document_embeddings: torch.Tensor) -> torch.Tensor:
        on_gpu = query_embeddings.is_cuda and document_embeddings.is_cuda
        needs_grad = torch.is_grad_enabled() and (query_embeddings.requires_grad or document_embeddings.requires_grad
                                                  or any(p.requires_grad for p in self.conv_layers.parameters()))
        if on_gpu and (self.native_backward or not needs_grad):
            convs = self._convs()
            ws, bs = [c.weight for c in convs], [c.bias for c in convs]
            try:
                if needs_grad:
                    flat = [x for p in self.pool_sizes for x in p]
                    return torch.ops.mm_native.matchpyramid_features_train(query_embeddings.float(),
                                                                           document_embeddings.float(), ws, bs, flat, 1)[0]
                return ops.matchpyramid_features(query_embeddings.float(), document_embeddings.float(), ws, bs,
                                                 self.pool_sizes, packed=self._packed_params(convs))
            except ops.NativeError as e:
                if getattr(e, "code", None) != _lib.MM_EUNSUPPORTED:
                    raise
        return self.torch_features(query_embeddings, document_embeddings)

    def forward(self, query_embeddings: torch.Tensor, document_embeddings: torch.Tensor,
                query_pad_oov_mask: torch.Tensor = None, document_pad_oov_mask: torch.Tensor = None,
                output_secondary_output: bool = False) -> torch.Tensor:
        conv_result_flat = self.features(query_embeddings, document_embeddings)
        dense_out = F.relu(self.dense(conv_result_flat))                                     # :99-101
        dense_out = F.relu(self.dense2(dense_out))
        dense_out = self.dense3(dense_out)
        output = torch.squeeze(dense_out, 1)
        if output_secondary_output:
            return output, {}
        return output

    def get_param_stats(self):
        return "MP: / "

    def get_param_secondary(self):
        return {}
