"""Host restatement (numpy) of the packed-caption row plan that vtp_text_row_plan builds on the device (vtp_amd/csrc/clip.hip): under the
causal mask with arg-max pooling only the tokens up to a caption's EOT are live, and the text tower stores them back to back."""
import numpy as np


def row_plan(ids):
    """ids [B, T] integer token ids -> (eot int32 [B], cu int32 [B + 1], rows int).
    eot[b] = position of the FIRST maximum of ids[b] (torch.argmax / text_global_pool 'argmax'); caption b has eot[b] + 1 live tokens and
    is the rows [cu[b], cu[b + 1]) of every packed buffer (cu = exclusive prefix sum of the lengths); rows = cu[B] = the live row count."""
    ids = np.asarray(ids)
    assert ids.ndim == 2 and ids.shape[0] > 0 and ids.shape[1] > 0
    eot = ids.argmax(axis=1).astype(np.int32)  # numpy's argmax returns the first maximum
    cu = np.zeros(ids.shape[0] + 1, dtype=np.int32)
    np.cumsum(eot.astype(np.int64) + 1, out=cu[1:])
    return eot, cu, int(cu[-1])


def packed_rows(cu, T):
    """int64 [rows]: padded row index b * T + t of every packed row, in packed order"""
    cu = np.asarray(cu, dtype=np.int64)
    return np.concatenate([b * T + np.arange(cu[b + 1] - cu[b]) for b in range(len(cu) - 1)])
