"""The intake the mini-batch ops share (sampling.py, subgraph.py, linkpred.py): the refusals that need no device work, worded once,
the seed draw, the stream-capture refusal and the leading arguments of every K22 / K23 / K24 entry point.  Private: the public names
stay in the three modules.  Each op keeps its own ORDER of refusals -- it calls these one by one."""
from __future__ import annotations

import torch

from .graph import CSRGraph, _stream    # noqa: F401  (the current stream, as graph.py hands it to its own entry points)

TRIM_FACTOR = 2            # buffers more than this many times the result are copied down to size


def _graph(op: str, graph) -> None:
    if not isinstance(graph, CSRGraph):
        raise ValueError(f"pygat_amd {op}: a CSRGraph expected, not {type(graph).__name__}")


def graph_head(graph: CSRGraph) -> tuple:
    """The four leading arguments of every entry point of the family."""
    return graph.n, graph.nnz, graph.fwd.rowptr.data_ptr(), graph.fwd.col.data_ptr()


def _hop(op: str, hop) -> None:
    if isinstance(hop, bool) or not isinstance(hop, int) or not 0 <= hop < 2 ** 32:
        raise ValueError(f"pygat_amd {op}: hop = {hop!r}: an int in [0, 2^32) expected")


def _at_least_one(op: str, name: str, value, expected: str = "an int >= 1 expected") -> int:
    """length, num_neg and a fanout that is not None: an int in [1, 2^31)."""
    if isinstance(value, bool) or not isinstance(value, int) or not 1 <= value < 2 ** 31:
        raise ValueError(f"pygat_amd {op}: {name} = {value!r}: {expected}")
    return value


def _seed(op: str, device, seed):
    if not isinstance(seed, torch.Tensor) or seed.dtype != torch.int64 or tuple(seed.shape) != (1,) or seed.device != device:
        got = f"{seed.dtype} {tuple(seed.shape)} on {seed.device}" if isinstance(seed, torch.Tensor) else type(seed).__name__
        raise ValueError(f"pygat_amd {op}: seed must be an int64 tensor of shape [1] on the graph's device {device} (the kernels read "
                         f"it there), got {got}")
    return seed.contiguous()


def _draw_seed(device, generator) -> torch.Tensor:
    """The seed of a call that was given none (inside torch.cuda.device(device))."""
    return torch.randint(0, 2 ** 62, (1,), dtype=torch.int64, device=device, generator=generator)


def _ids(op: str, graph, ids, name: str, shape: str, limit: bool = True):
    """Every refusal of a list of node ids that needs no device work -> int64 contiguous.  limit=False: dst, whose count is held
    against the graph's node count instead ("some id repeats")."""
    _graph(op, graph)
    if not isinstance(ids, torch.Tensor) or not ids.is_cuda:
        raise ValueError(f"pygat_amd {op}: {name} must be a tensor on the GPU (there is no CPU path)")
    if ids.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"pygat_amd {op}: {name} must be int32 or int64, not {ids.dtype}")
    if ids.dim() != 1 or ids.numel() < 1:
        raise ValueError(f"pygat_amd {op}: {name} [{shape}] with {shape} >= 1 expected, got {tuple(ids.shape)}")
    if ids.device != graph.device:
        raise ValueError(f"pygat_amd {op}: {name} lives on {ids.device}, the graph on {graph.device}")
    if limit and ids.numel() >= 2 ** 31:
        raise ValueError(f"pygat_amd {op}: {name} holds {ids.numel()} ids: fewer than 2^31 expected")
    return ids.to(torch.int64).contiguous()


def _no_capture(op: str, what: str, read_back: str, instead: str) -> None:
    """Every op of the family ends in a host read, so none runs during stream capture."""
    if torch.cuda.is_current_stream_capturing():
        raise ValueError(f"pygat_amd {op}: {what} during stream capture ({read_back} read back); {instead} before the capture")


def _trim(t: torch.Tensor, n: int) -> torch.Tensor:
    return t[:n].clone() if t.shape[0] > TRIM_FACTOR * max(n, 1) else t[:n]
