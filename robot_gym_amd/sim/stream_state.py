"""What DomainRandomizer, SensorModel and StateEstimator share on the Python side of the stream of include/rg_stream.h: the
state table a bind() makes and the column copy behind copy_columns."""
import torch


def stream_state(rows, batch, device):
    """float64 [rows, batch] zeros with row 0, the robot's key in the stream, = arange(batch)."""
    state = torch.zeros(rows, batch, dtype=torch.float64, device=device)
    state[0] = torch.arange(batch, dtype=torch.float64, device=device)
    return state


def copy_robot_columns(tensors_and_dims, src, dst, index):
    """For every (tensor, dim): the entries src[k] along dim into the entries dst[k] (all sources read first).  index turns
    src and dst into int64 index tensors of the tensors' device.  Returns the dst index tensor."""
    s, t = index(src), index(dst)
    if s.numel() != t.numel():
        raise ValueError("copy_columns: src and dst differ in length")
    for ten, dim in tensors_and_dims:
        ten.index_copy_(dim, t, ten.index_select(dim, s))
    return t
