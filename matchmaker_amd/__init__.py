"""matchmaker_amd — MI355X-native (gfx950) interaction scoring for matchmaker's re-ranking forward
pass: ColBERT MaxSim and TK / TKL kernel pooling as hand-written HIP kernels behind the reference's
own model interface.  See DESIGN.md / INTEGRATION.md."""
from ._lib import NativeError, LIB_PATH  # noqa: F401
from . import ops  # noqa: F401

__all__ = ["ops", "NativeError", "LIB_PATH", "FlatIPIndexer", "IVFFlatIPIndexer", "DynamicIVFIndexer", "GraphIPIndexer", "ScannIPIndexer",
           "MaxPIndexer", "TokenStore", "TokenStoreWriter", "encode_collection", "fp8_quantize_rows", "fp8_dequantize_rows", "maxsim_ragged_fp8",
           "losses", "get_loss", "patch_losses", "inbatch", "InBatchNegatives", "contextualize"]


def __getattr__(name):          # the indexers, imported on first use (retrieval pulls in torch.distributed)
    if name in ("FlatIPIndexer", "IVFFlatIPIndexer", "DynamicIVFIndexer", "GraphIPIndexer", "ScannIPIndexer", "MaxPIndexer"):
        from . import retrieval
        return getattr(retrieval, name)
    if name == "TokenStore":    # the ColBERT token store (16-bit, or fp8: TokenStore.quantize_fp8 / load(..., fp8=True))
        from .token_store import TokenStore
        return TokenStore
    if name == "TokenStoreWriter":   # the device-side writer of that store (encoder output -> TokenStore)
        from .token_store import TokenStoreWriter
        return TokenStoreWriter
    if name == "encode_collection":
        from .encode import encode_collection
        return encode_collection
    if name in ("fp8_quantize_rows", "fp8_dequantize_rows", "maxsim_ragged_fp8"):   # the fp8 store's operators
        return getattr(ops, name)
    if name == "losses":        # the native training losses (drop-ins for matchmaker/losses/*.py) and their get_loss
        import importlib
        return importlib.import_module(".losses", __name__)
    if name == "inbatch":       # the native in-batch negatives of dense-retriever training (train.py:434-472)
        import importlib
        return importlib.import_module(".inbatch", __name__)
    if name == "contextualize":  # the TK-family contextualiser with its attention core on csrc/self_attention.hip
        import importlib
        return importlib.import_module(".contextualize", __name__)
    if name == "InBatchNegatives":
        from .inbatch import InBatchNegatives
        return InBatchNegatives
    if name == "get_loss":
        from .losses import get_loss
        return get_loss
    if name == "patch_losses":  # opt-in: patch_matchmaker() rebinds the models only
        from .patch import patch_losses
        return patch_losses
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
