"""The model-facing part of the reference's encode loop (matchmaker/dense_retrieval.py:224-280) over a TokenStoreWriter.

The reference runs `model_indexer.forward(batch["seq_tokens"])` (CollectionIndexerHead.forward,
matchmaker/modules/indexing_heads.py:20-27: `forward_representation(seq, sequence_type="doc_encode")` under autocast),
copies the padded output to the CPU and compacts it there document by document.  Here the output stays on the device and
`writer.append` compacts it into the resident store (ops.store_append).
"""
import torch

from .token_store import TokenStoreWriter


def encode_collection(model, batches, writer: TokenStoreWriter, use_fp16: bool = True) -> int:
    """For every batch of `batches` (dicts with "seq_tokens" and "seq_id", already on the model's device, as the reference's
    loader yields them after move_to_device): vecs = model.forward_representation(batch["seq_tokens"],
    sequence_type="doc_encode") under autocast(enabled=use_fp16), then writer.append(batch["seq_id"], vecs).
    Returns the number of sequences encoded; writer.finish() gives the store."""
    n = 0
    with torch.no_grad():
        for batch in batches:
            with torch.autocast("cuda", enabled=use_fp16):
                vecs = model.forward_representation(batch["seq_tokens"], sequence_type="doc_encode")
            writer.append(batch["seq_id"], vecs)
            n += len(batch["seq_id"])
    return n
