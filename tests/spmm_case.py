"""Ground truth and inputs of the tests of pygat_amd.spmm (csrc/k17_spmm.hip): the product through torch autograd on the CPU, in
any dtype, and seeded input generators.  Imported by tests/test_gpu_spmm.py."""
import numpy as np
import torch


def spmm_ref(row, col, n_rows, values, b):
    """values [E] | [E, H], b [M, F] | [M, H, F] -> out [n_rows, F] | [n_rows, H, F]: every entry adds values[k] * b[col[k]] to
    row[k] (repeated pairs add, as torch.sparse_coo_tensor's do)."""
    v = values if values.dim() == 2 else values[:, None]
    t = b if b.dim() == 3 else b[:, None, :]
    out = torch.zeros(n_rows, t.shape[1], t.shape[2], dtype=t.dtype).index_add(0, row, v[:, :, None] * t[col])
    return out if b.dim() == 3 else out[:, 0]


def coo_of(rowptr, col):
    """CSR -> (row, col) int64 tensors in CSR order."""
    rp = torch.as_tensor(np.asarray(rowptr), dtype=torch.int64)
    return torch.repeat_interleave(torch.arange(rp.numel() - 1), rp[1:] - rp[:-1]), torch.as_tensor(np.asarray(col), dtype=torch.int64)


def softmax_values(row, n_rows, H, seed):
    """[E, H] float64: a softmax over the entries of every row of N(0, 1) logits -- the op's real use (layers.py:145-150)."""
    g = torch.Generator().manual_seed(seed)
    e = torch.randn(row.numel(), H, generator=g, dtype=torch.float64)
    m = torch.full((n_rows, H), -float("inf"), dtype=torch.float64).scatter_reduce(0, row[:, None].expand(-1, H), e, "amax")
    p = torch.exp(e - m[row])
    return p / torch.zeros(n_rows, H, dtype=torch.float64).index_add(0, row, p)[row]


def normal(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def f32(t):
    """The fp32 rounding of a float64 tensor, as float64: what both the device and the ground truth are fed."""
    return t.float().double()
