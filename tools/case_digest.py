#!/usr/bin/env python3
"""One line per seeded case of the case modules named on the command line: `<module> <case name> <sha256>`.

The hash covers a case's attributes in sorted name order: a tensor or an ndarray gives its dtype, shape and bytes, a Python
scalar or string its repr, a list or tuple its items in turn; anything else gives its type's name only.  A test refactor that
moves no seed, draw order, grid rounding or kink assert leaves the output byte-identical; the tool imports nothing of pygat_amd,
so a copy of it beside a checkout of another commit digests that commit's cases.

    python tools/case_digest.py dot_attention_case spmm_case ... | sha256sum
"""
import hashlib
import importlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path[:0] = [os.path.join(ROOT, "tests"), ROOT]            # the case modules, and the oracle package their graphs come from


def feed(h, v):
    if isinstance(v, torch.Tensor):
        h.update(f"{v.dtype}{tuple(v.shape)}".encode() + v.detach().contiguous().reshape(-1).view(torch.uint8).numpy().tobytes())
    elif isinstance(v, np.ndarray):
        h.update(f"{v.dtype}{v.shape}".encode() + np.ascontiguousarray(v).tobytes())
    elif isinstance(v, (bool, int, float, str, type(None))):
        h.update(repr(v).encode())
    elif isinstance(v, (list, tuple)):
        h.update(f"{type(v).__name__}{len(v)}".encode())
        for item in v:
            feed(h, item)
    else:
        h.update(type(v).__name__.encode())


for module in sys.argv[1:]:
    for name, case in getattr(importlib.import_module(module), "cases", dict)().items():
        h = hashlib.sha256()
        for attr in sorted(vars(case)):
            h.update(attr.encode())
            feed(h, vars(case)[attr])
        print(module, name, h.hexdigest())
