"""The refusals of the pattern ops (pygat_amd/spmm.py, edge_softmax.py, dot_attention.py, additive_attention.py, gatv2_attention.py),
most of them made through their shared intake (pygat_amd/_pattern_ops.py), word for word: no GPU is needed, an EdgePattern that was
never built stands in for the pattern and CPU tensors that claim to be on the GPU for the tables -- every refusal is raised before
anything touches a device.  EXPECTED was recorded from the commit before the intake was shared, never from the code under test: the
messages are behaviour, and so is the order in which two bad arguments are refused."""
import pytest
import torch

R, C, E = 5, 7, 11                                                   # rows, columns and entries of the stand-in; H = 2, F = 8
F32, BF16 = torch.float32, torch.bfloat16


class OnGpu(torch.Tensor):
    is_cuda = property(lambda self: True)


def _gpu(t):
    return t.as_subclass(OnGpu)


def _t(*dims, dtype=F32, grad=False):
    return _gpu(torch.zeros(*dims, dtype=dtype, requires_grad=grad))


def _pattern(device="cpu"):
    """An EdgePattern that was never built: enough for the refusals made before any of its arrays is touched."""
    import pygat_amd as pg
    p = object.__new__(pg.EdgePattern)
    p.shape, p.n_rows, p.n_cols, p.nnz, p.device, p._t = (R, C), R, C, E, torch.device(device), None
    return p


def _hf(H, F, flat):
    return (F,) if flat else (H, F)


def _h(H, flat):
    return () if flat else (H,)


# ---- the good arguments of every op, by name, at H heads of width F (flat: without a head axis)
def _spmm(H=2, F=8, flat=False):
    return dict(pattern=_pattern(), values=_t(E, *_h(H, flat)), b=_t(C, *_hf(H, F, flat)))


def _edge_softmax(H=2, F=8, flat=False):
    return dict(pattern=_pattern(), logits=_t(E, *_h(H, flat)))


def _edge_dot(H=2, F=8, flat=False):
    return dict(pattern=_pattern(), q=_t(R, *_hf(H, F, flat)), k=_t(C, *_hf(H, F, flat)))


def _dot(H=2, F=8, flat=False, kv=F32, bias=False, e=False, p=False):
    s = _hf(H, F, flat)
    a = dict(pattern=_pattern(), q=_t(R, *s), k=_t(C, *s, dtype=kv), v=_t(C, *s, dtype=kv))
    if e:
        a["e"] = _t(E, *s)
    if p:
        a["p"] = 0.5
    if bias:
        a["bias"] = _t(E, *_h(H, flat))
    return a


def _additive(H=2, F=8, flat=False, v=F32, logit=False, p=False):
    a = dict(pattern=_pattern(), s_dst=_t(R, *_h(H, flat)), s_src=_t(C, *_h(H, flat)))
    a["v16" if v == BF16 else "v"] = _t(C, *_hf(H, F, flat), dtype=v)
    if p:
        a["p"] = 0.5
    if logit:
        a["edge_logit"] = _t(E, *_h(H, flat))
    return a


def _gatv2(H=2, F=8, flat=False, tables=F32, v=False, e=False, p=False):
    s, sfx = _hf(H, F, flat), "16" if tables == BF16 else ""
    a = dict(pattern=_pattern(), x_dst=_t(R, *s), a=_t(*s))
    a["x_src" + sfx] = _t(C, *s, dtype=tables)
    if e:
        a["e" + sfx] = _t(E, *s, dtype=tables)
    if p:
        a["p"] = 0.5
    if v:
        a["v" + sfx] = _t(C, *s, dtype=tables)
    return a


def _mask(H=2, F=8, flat=False):
    return dict(pattern=_pattern(), H=H, p=0.5, seed=torch.zeros(1, dtype=torch.int64))


def _with(good, **fixed):
    return lambda **kw: good(**fixed, **kw)


LIMITS = (("H = 65", dict(H=65, F=4)), ("F = 12", dict(F=12)), ("F = 2", dict(F=2)), ("F = 512", dict(F=512)),
          ("H * F = 2048", dict(H=8, F=256)))

# op -> (its good arguments, the tensors whose leading size is held against the pattern, which LIMITS it has)
OPS = {
    "spmm": (_spmm, ("values", "b"), ("H = 65", "H * F = 2048")),
    "edge_softmax": (_edge_softmax, ("logits",), ("H = 65",)),
    "edge_dot": (_edge_dot, ("q", "k"), ("H = 65", "H * F = 2048")),
    "dot_attention": (_dot, ("q", "k", "v"), None),
    "dot_attention.bias": (_with(_dot, bias=True), ("q", "k", "v", "bias"), None),
    "dot_attention.bf16": (_with(_dot, kv=BF16, bias=True), ("q", "k", "v", "bias"), None),
    "dot_attention_dropout": (_with(_dot, bias=True, p=True), ("q", "k", "v", "bias"), None),
    "dot_attention_edge": (_with(_dot, bias=True, e=True), ("q", "k", "v", "e", "bias"), None),
    "additive_attention": (_with(_additive, logit=True), ("s_dst", "s_src", "v", "edge_logit"), None),
    "additive_attention_dropout": (_with(_additive, logit=True, p=True), ("s_dst", "s_src", "v", "edge_logit"), None),
    "additive_attention_bf16": (_with(_additive, logit=True, v=BF16), ("s_dst", "s_src", "v16", "edge_logit"), None),
    "gatv2_attention": (_with(_gatv2, v=True), ("x_dst", "x_src", "v"), None),
    "gatv2_attention.shared": (_gatv2, ("x_dst", "x_src"), None),
    "gatv2_attention_dropout": (_with(_gatv2, v=True, p=True), ("x_dst", "x_src", "v"), None),
    "gatv2_attention_edge": (_with(_gatv2, v=True, e=True), ("x_dst", "x_src", "e", "v"), None),
    "gatv2_attention_bf16": (_with(_gatv2, v=True, tables=BF16), ("x_dst", "x_src16", "v16"), None),
    "gatv2_attention_edge_bf16": (_with(_gatv2, v=True, e=True, tables=BF16), ("x_dst", "x_src16", "e16", "v16"), None),
    "attention_dropout_mask": (_mask, (), ("H = 65",)),
}


def _call(op, args):
    import pygat_amd as pg
    return getattr(pg, op.split(".")[0])(**args)


def _cases(op):
    """(case name, the arguments) of every refusal of `op` that looks at nothing but the arguments."""
    good, sized, limits = OPS[op]
    yield "no pattern", dict(good(), pattern=object())
    yield "another device", dict(good(), pattern=_pattern("cuda:1"))
    tensors = [n for n, t in good().items() if isinstance(t, OnGpu)]
    for name in tensors:
        t = good()[name]
        other = F32 if t.dtype == BF16 else BF16
        yield f"{name} no tensor", dict(good(), **{name: [1.0]})
        yield f"{name} on the cpu", dict(good(), **{name: torch.zeros(t.shape, dtype=t.dtype)})
        yield f"{name} float64", dict(good(), **{name: _t(*t.shape, dtype=torch.float64)})
        yield f"{name} {other}", dict(good(), **{name: _t(*t.shape, dtype=other)})
        yield f"{name} one more dimension", dict(good(), **{name: _t(*t.shape, 1, dtype=t.dtype)})
        if tuple(t.shape) != tuple(good(H=3)[name].shape) and op != "edge_softmax":          # (its H is the logits')
            yield f"{name} of 3 heads", dict(good(), **{name: good(H=3)[name]})
        if tuple(t.shape) != tuple(good(F=4)[name].shape) and not op.startswith(("spmm", "additive")):   # (their F is one table's)
            yield f"{name} of F = 4", dict(good(), **{name: good(F=4)[name]})
        if name in sized:
            yield f"{name} one more row", dict(good(), **{name: _t(t.shape[0] + 1, *t.shape[1:], dtype=t.dtype)})
    for name, hf in LIMITS:
        if limits is None or name in limits:
            yield name, good(**hf)
    if op == "attention_dropout_mask":
        yield "H True", dict(good(), H=True)
    for name in ("bias", "edge_logit"):                              # [E, H] | [E]; [E] alone without a head axis
        if name in good():
            yield f"{name} [E, 1] beside heads", dict(good(), **{name: _t(E, 1)})
            yield f"{name} [E, H] without a head axis", dict(good(flat=True), **{name: _t(E, 2)})
    if "p" in good():
        for bad in (-0.1, 1.5, True, float("nan")):
            yield f"p {bad!r}", dict(good(), p=bad)
    if "p" in good() or op == "attention_dropout_mask":
        yield "seed dtype", dict(good(), seed=torch.zeros(1, dtype=torch.int32))
        yield "seed shape", dict(good(), seed=torch.zeros(2, dtype=torch.int64))
        yield "seed no tensor", dict(good(), seed=7)
    if op.startswith(("additive", "gatv2")):
        for bad in (True, float("inf")):
            yield f"negative_slope {bad!r}", dict(good(), negative_slope=bad)
    if op.endswith("bf16"):
        for name in tensors:
            t = good()[name]
            yield f"{name} requires grad", dict(good(), **{name: _t(*t.shape, dtype=t.dtype, grad=True)})


def _two(good, **bad):
    return lambda: dict(good(), **bad)


BAD_SEED = torch.zeros(2, dtype=torch.int64)

# two bad arguments at once: the one refused first
ORDER = {
    "dot_attention: bias before q": ("dot_attention", _two(_dot, bias=_t(E, 2, dtype=torch.float64), q=[1.0])),
    "dot_attention: q's dtype before k's shape": ("dot_attention", _two(_dot, q=_t(R, 2, 8, dtype=torch.float64), k=_t(C, 3, 8))),
    "dot_attention: k's shape before q's rows": ("dot_attention", _two(_dot, k=_t(C, 3, 8), q=_t(R + 1, 2, 8))),
    "dot_attention: q's rows before the bias's shape": ("dot_attention", _two(_dot, q=_t(R + 1, 2, 8), bias=_t(E, 3))),
    "dot_attention: F before the bias's shape": ("dot_attention", lambda: dict(_dot(F=12), bias=_t(E, 3))),
    "dot_attention: one bf16 table before no pattern": ("dot_attention", _two(_dot, k=_t(C, 2, 8, dtype=BF16), pattern=None)),
    "dot_attention.bf16: requires grad before no pattern": ("dot_attention", _two(_with(_dot, kv=BF16), q=_t(R, 2, 8, grad=True),
                                                                                  pattern=None)),
    "dot_attention_dropout: a bf16 v before p": ("dot_attention_dropout", _two(_with(_dot, p=True), v=_t(C, 2, 8, dtype=BF16), p=1.5)),
    "dot_attention_dropout: p before the seed": ("dot_attention_dropout", _two(_with(_dot, p=True), p=1.5, seed=BAD_SEED)),
    "dot_attention_dropout: the seed before q": ("dot_attention_dropout", _two(_with(_dot, p=True), seed=BAD_SEED, q=[1.0])),
    "dot_attention_dropout: q before training=False": ("dot_attention_dropout", _two(_with(_dot, p=True), q=[1.0], training=False)),
    "dot_attention_edge: a bf16 e before no pattern": ("dot_attention_edge", _two(_with(_dot, e=True), e=_t(E, 2, 8, dtype=BF16),
                                                                                 pattern=None)),
    "dot_attention_edge: e's dtype before the bias": ("dot_attention_edge", _two(_with(_dot, e=True), e=_t(E, 2, 8, dtype=torch.float64),
                                                                                bias=[1.0])),
    "dot_attention_edge: q before e's shape": ("dot_attention_edge", _two(_with(_dot, e=True), e=_t(E + 1, 2, 8), q=_t(R + 1, 2, 8))),
    "dot_attention_edge: the bias's shape before e's": ("dot_attention_edge", _two(_with(_dot, e=True), e=_t(E + 1, 2, 8), bias=_t(E, 3))),
    "additive_attention: the slope before the logit": ("additive_attention", _two(_additive, negative_slope=True, edge_logit=[1.0])),
    "additive_attention: the logit before s_dst": ("additive_attention", _two(_additive, edge_logit=[1.0], s_dst=[1.0])),
    "additive_attention: v's shape before s_dst's rows": ("additive_attention", _two(_additive, v=_t(C, 3, 8), s_dst=_t(R + 1, 2))),
    "additive_attention: F before the logit's shape": ("additive_attention", lambda: dict(_additive(F=12), edge_logit=_t(E, 3))),
    "additive_attention_dropout: a bf16 v before p": ("additive_attention_dropout", _two(_with(_additive, p=True), v=_t(C, 2, 8, dtype=BF16),
                                                                                        p=1.5)),
    "additive_attention_dropout: p before the slope": ("additive_attention_dropout", _two(_with(_additive, p=True), p=1.5,
                                                                                         negative_slope=True)),
    "additive_attention_dropout: the slope before the seed": ("additive_attention_dropout", _two(_with(_additive, p=True),
                                                                                                negative_slope=True, seed=BAD_SEED)),
    "additive_attention_dropout: the seed before s_dst": ("additive_attention_dropout", _two(_with(_additive, p=True), seed=BAD_SEED,
                                                                                            s_dst=[1.0])),
    "additive_attention_bf16: the slope before requires grad": ("additive_attention_bf16", _two(_with(_additive, v=BF16),
                                                                                               negative_slope=True, s_dst=_t(R, 2, grad=True))),
    "additive_attention_bf16: requires grad before a float32 v16": ("additive_attention_bf16", _two(_with(_additive, v=BF16),
                                                                                                   s_dst=_t(R, 2, grad=True), v16=_t(C, 2, 8))),
    "additive_attention_bf16: a float32 v16 before no pattern": ("additive_attention_bf16", _two(_with(_additive, v=BF16), v16=_t(C, 2, 8),
                                                                                                pattern=None)),
    "gatv2_attention: the slope before x_dst": ("gatv2_attention", _two(_gatv2, negative_slope=True, x_dst=[1.0])),
    "gatv2_attention: v's shape before a's": ("gatv2_attention", _two(_gatv2, v=_t(C, 3, 8), a=_t(2, 4))),
    "gatv2_attention: a's shape before x_dst's rows": ("gatv2_attention", _two(_gatv2, a=_t(2, 4), x_dst=_t(R + 1, 2, 8))),
    "gatv2_attention_dropout: a bf16 a before p": ("gatv2_attention_dropout", _two(_with(_gatv2, p=True), a=_t(2, 8, dtype=BF16), p=1.5)),
    "gatv2_attention_dropout: p before the slope": ("gatv2_attention_dropout", _two(_with(_gatv2, p=True), p=1.5, negative_slope=True)),
    "gatv2_attention_dropout: the slope before the seed": ("gatv2_attention_dropout", _two(_with(_gatv2, p=True), negative_slope=True,
                                                                                          seed=BAD_SEED)),
    "gatv2_attention_dropout: the seed before x_dst": ("gatv2_attention_dropout", _two(_with(_gatv2, p=True), seed=BAD_SEED, x_dst=[1.0])),
    "gatv2_attention_edge: a bf16 e before the slope": ("gatv2_attention_edge", _two(_with(_gatv2, e=True), e=_t(E, 2, 8, dtype=BF16),
                                                                                    negative_slope=True)),
    "gatv2_attention_edge: the slope before e": ("gatv2_attention_edge", _two(_with(_gatv2, e=True), negative_slope=True, e=[1.0])),
    "gatv2_attention_edge: e's dtype before x_dst": ("gatv2_attention_edge", _two(_with(_gatv2, e=True), e=_t(E, 2, 8, dtype=torch.float64),
                                                                                 x_dst=[1.0])),
    "gatv2_attention_edge: x_dst's rows before e's shape": ("gatv2_attention_edge", _two(_with(_gatv2, e=True), e=_t(E + 1, 2, 8),
                                                                                        x_dst=_t(R + 1, 2, 8))),
    "gatv2_attention_edge: F before e's shape": ("gatv2_attention_edge", lambda: dict(_gatv2(F=12, e=True), e=_t(E + 1, 2, 12))),
    "gatv2_attention_edge_bf16: the slope before requires grad": ("gatv2_attention_edge_bf16", _two(_with(_gatv2, e=True, tables=BF16),
                                                                                                   negative_slope=True, a=_t(2, 8, grad=True))),
    "gatv2_attention_edge_bf16: requires grad before a float32 e16": ("gatv2_attention_edge_bf16", _two(_with(_gatv2, e=True, tables=BF16),
                                                                                                       a=_t(2, 8, grad=True), e16=_t(E, 2, 8))),
    "gatv2_attention_edge_bf16: a float32 e16 before no pattern": ("gatv2_attention_edge_bf16", _two(_with(_gatv2, e=True, tables=BF16),
                                                                                                    e16=_t(E, 2, 8), pattern=None)),
    "gatv2_attention_edge_bf16: e16 no tensor before x_dst": ("gatv2_attention_edge_bf16", _two(_with(_gatv2, e=True, tables=BF16),
                                                                                               e16=None, x_dst=[1.0])),
    "gatv2_attention_edge_bf16: x_dst's rows before e16's shape": ("gatv2_attention_edge_bf16", _two(_with(_gatv2, e=True, tables=BF16),
                                                                                                    x_dst=_t(R + 1, 2, 8),
                                                                                                    e16=_t(E + 1, 2, 8, dtype=BF16))),
    "spmm: values before b": ("spmm", _two(_spmm, values=[1.0], b=[1.0])),
    "spmm: b's dtype before the shapes": ("spmm", _two(_spmm, b=_t(C, 2, 8, dtype=torch.float64), values=_t(E, 3))),
    "spmm: the shapes before the entries": ("spmm", _two(_spmm, b=_t(C, 3, 8), values=_t(E + 1, 2))),
    "edge_softmax: no pattern before by": ("edge_softmax", _two(_edge_softmax, pattern=None, by="both")),
    "edge_softmax: by before the logits": ("edge_softmax", _two(_edge_softmax, by="both", logits=[1.0])),
    "edge_dot: q before k": ("edge_dot", _two(_edge_dot, q=[1.0], k=[1.0])),
    "edge_dot: k's shape before q's rows": ("edge_dot", _two(_edge_dot, k=_t(C, 3, 8), q=_t(R + 1, 2, 8))),
    "attention_dropout_mask: p before the seed before H": ("attention_dropout_mask", _two(_mask, p=1.5, seed=BAD_SEED, H=65)),
    "attention_dropout_mask: the seed before H": ("attention_dropout_mask", _two(_mask, seed=BAD_SEED, H=65)),
}


def _refusal(op, args):
    with pytest.raises(ValueError) as e:
        _call(op, args)
    return str(e.value)


EXPECTED = {'spmm': {'no pattern': 'pygat_amd spmm: an EdgePattern expected (EdgePattern.from_indices, CSRGraph.edge_pattern)',
          'another device': 'pygat_amd spmm: values lives on cpu, the pattern on cuda:1',
          'values no tensor': 'pygat_amd spmm: values must be a tensor on the GPU (there is no CPU path)',
          'values on the cpu': 'pygat_amd spmm: values must be a tensor on the GPU (there is no CPU path)',
          'values float64': 'pygat_amd spmm: values must be float32, not torch.float64',
          'values torch.bfloat16': 'pygat_amd spmm: values must be float32, not torch.bfloat16',
          'values one more dimension': 'pygat_amd spmm: values [E] with b [M, F], or values [E, H] with b [M, H, F], expected; got values (11, 2, 1) '
                                       'and b (7, 2, 8)',
          'values of 3 heads': 'pygat_amd spmm: values [E] with b [M, F], or values [E, H] with b [M, H, F], expected; got values (11, 3) and b (7, '
                               '2, 8)',
          'values one more row': 'pygat_amd spmm: values has 12 rows but the pattern has 11 entries',
          'b no tensor': 'pygat_amd spmm: b must be a tensor on the GPU (there is no CPU path)',
          'b on the cpu': 'pygat_amd spmm: b must be a tensor on the GPU (there is no CPU path)',
          'b float64': 'pygat_amd spmm: b must be float32, not torch.float64',
          'b torch.bfloat16': 'pygat_amd spmm: b must be float32, not torch.bfloat16',
          'b one more dimension': 'pygat_amd spmm: values [E] with b [M, F], or values [E, H] with b [M, H, F], expected; got values (11, 2) and b '
                                  '(7, 2, 8, 1)',
          'b of 3 heads': 'pygat_amd spmm: values [E] with b [M, F], or values [E, H] with b [M, H, F], expected; got values (11, 2) and b (7, 3, 8)',
          'b one more row': 'pygat_amd spmm: b has 8 rows but the pattern has 7 columns',
          'H = 65': 'pygat_amd spmm: H = 65 heads of F = 4 columns: the limits are 1 <= H <= 64, F >= 1 and H * F <= 1024 floats per row',
          'H * F = 2048': 'pygat_amd spmm: H = 8 heads of F = 256 columns: the limits are 1 <= H <= 64, F >= 1 and H * F <= 1024 floats per row'},
 'edge_softmax': {'no pattern': 'pygat_amd edge_softmax: an EdgePattern expected (EdgePattern.from_indices, CSRGraph.edge_pattern)',
                  'another device': 'pygat_amd edge_softmax: logits lives on cpu, the pattern on cuda:1',
                  'logits no tensor': 'pygat_amd edge_softmax: logits must be a tensor on the GPU (there is no CPU path)',
                  'logits on the cpu': 'pygat_amd edge_softmax: logits must be a tensor on the GPU (there is no CPU path)',
                  'logits float64': 'pygat_amd edge_softmax: logits must be float32, not torch.float64',
                  'logits torch.bfloat16': 'pygat_amd edge_softmax: logits must be float32, not torch.bfloat16',
                  'logits one more dimension': 'pygat_amd edge_softmax: logits [E] or [E, H] expected, got (11, 2, 1)',
                  'logits one more row': 'pygat_amd edge_softmax: logits has 12 rows but the pattern has 11 entries',
                  'H = 65': 'pygat_amd edge_softmax: H = 65 heads: the limits are 1 <= H <= 64'},
 'edge_dot': {'no pattern': 'pygat_amd edge_dot: an EdgePattern expected (EdgePattern.from_indices, CSRGraph.edge_pattern)',
              'another device': 'pygat_amd edge_dot: q lives on cpu, the pattern on cuda:1',
              'q no tensor': 'pygat_amd edge_dot: q must be a tensor on the GPU (there is no CPU path)',
              'q on the cpu': 'pygat_amd edge_dot: q must be a tensor on the GPU (there is no CPU path)',
              'q float64': 'pygat_amd edge_dot: q must be float32, not torch.float64',
              'q torch.bfloat16': 'pygat_amd edge_dot: q must be float32, not torch.bfloat16',
              'q one more dimension': 'pygat_amd edge_dot: q [n_rows, F] or [n_rows, H, F] expected, got (5, 2, 8, 1)',
              'q of 3 heads': 'pygat_amd edge_dot: k (7, 2, 8) does not match q (5, 3, 8): the same number of heads and the same F expected',
              'q of F = 4': 'pygat_amd edge_dot: k (7, 2, 8) does not match q (5, 2, 4): the same number of heads and the same F expected',
              'q one more row': 'pygat_amd edge_dot: q has 6 rows but the pattern has 5 rows',
              'k no tensor': 'pygat_amd edge_dot: k must be a tensor on the GPU (there is no CPU path)',
              'k on the cpu': 'pygat_amd edge_dot: k must be a tensor on the GPU (there is no CPU path)',
              'k float64': 'pygat_amd edge_dot: k must be float32, not torch.float64',
              'k torch.bfloat16': 'pygat_amd edge_dot: k must be float32, not torch.bfloat16',
              'k one more dimension': 'pygat_amd edge_dot: k (7, 2, 8, 1) does not match q (5, 2, 8): the same number of heads and the same F '
                                      'expected',
              'k of 3 heads': 'pygat_amd edge_dot: k (7, 3, 8) does not match q (5, 2, 8): the same number of heads and the same F expected',
              'k of F = 4': 'pygat_amd edge_dot: k (7, 2, 4) does not match q (5, 2, 8): the same number of heads and the same F expected',
              'k one more row': 'pygat_amd edge_dot: k has 8 rows but the pattern has 7 columns',
              'H = 65': 'pygat_amd edge_dot: H = 65 heads of F = 4 columns: the limits are 1 <= H <= 64, F >= 1 and H * F <= 1024 floats per row',
              'H * F = 2048': 'pygat_amd edge_dot: H = 8 heads of F = 256 columns: the limits are 1 <= H <= 64, F >= 1 and H * F <= 1024 floats per '
                              'row'},
 'dot_attention': {'no pattern': 'pygat_amd dot_attention: an EdgePattern expected (EdgePattern.from_indices, CSRGraph.edge_pattern)',
                   'another device': 'pygat_amd dot_attention: q lives on cpu, the pattern on cuda:1',
                   'q no tensor': 'pygat_amd dot_attention: q must be a tensor on the GPU (there is no CPU path)',
                   'q on the cpu': 'pygat_amd dot_attention: q must be a tensor on the GPU (there is no CPU path)',
                   'q float64': 'pygat_amd dot_attention: q must be float32, not torch.float64',
                   'q torch.bfloat16': 'pygat_amd dot_attention: q must be float32, not torch.bfloat16',
                   'q one more dimension': 'pygat_amd dot_attention: q [n_rows, F] or [n_rows, H, F] expected, got (5, 2, 8, 1)',
                   'q of 3 heads': 'pygat_amd dot_attention: k (7, 2, 8) does not match q (5, 3, 8): the same number of heads and the same F '
                                   'expected',
                   'q of F = 4': 'pygat_amd dot_attention: k (7, 2, 8) does not match q (5, 2, 4): the same number of heads and the same F expected',
                   'q one more row': 'pygat_amd dot_attention: q has 6 rows but the pattern has 5 rows',
                   'k no tensor': 'pygat_amd dot_attention: k must be a tensor on the GPU (there is no CPU path)',
                   'k on the cpu': 'pygat_amd dot_attention: k must be a tensor on the GPU (there is no CPU path)',
                   'k float64': 'pygat_amd dot_attention: k must be float32, not torch.float64',
                   'k torch.bfloat16': 'pygat_amd dot_attention: k is torch.bfloat16 and v is torch.float32: the inference forward takes both k and '
                                       'v as bfloat16 tables (k.bfloat16(), v.bfloat16()); otherwise both are float32',
                   'k one more dimension': 'pygat_amd dot_attention: k (7, 2, 8, 1) does not match q (5, 2, 8): the same number of heads and the '
                                           'same F expected',
                   'k of 3 heads': 'pygat_amd dot_attention: k (7, 3, 8) does not match q (5, 2, 8): the same number of heads and the same F '
                                   'expected',
                   'k of F = 4': 'pygat_amd dot_attention: k (7, 2, 4) does not match q (5, 2, 8): the same number of heads and the same F expected',
                   'k one more row': 'pygat_amd dot_attention: k has 8 rows but the pattern has 7 columns',
                   'v no tensor': 'pygat_amd dot_attention: v must be a tensor on the GPU (there is no CPU path)',
                   'v on the cpu': 'pygat_amd dot_attention: v must be a tensor on the GPU (there is no CPU path)',
                   'v float64': 'pygat_amd dot_attention: v must be float32, not torch.float64',
                   'v torch.bfloat16': 'pygat_amd dot_attention: k is torch.float32 and v is torch.bfloat16: the inference forward takes both k and '
                                       'v as bfloat16 tables (k.bfloat16(), v.bfloat16()); otherwise both are float32',
                   'v one more dimension': 'pygat_amd dot_attention: v (7, 2, 8, 1) does not match q (5, 2, 8): the same number of heads and the '
                                           'same F expected',
                   'v of 3 heads': 'pygat_amd dot_attention: v (7, 3, 8) does not match q (5, 2, 8): the same number of heads and the same F '
                                   'expected',
                   'v of F = 4': 'pygat_amd dot_attention: v (7, 2, 4) does not match q (5, 2, 8): the same number of heads and the same F expected',
                   'v one more row': 'pygat_amd dot_attention: v has 8 rows but the pattern has 7 columns',
                   'H = 65': 'pygat_amd dot_attention: H = 65 heads: the limits are 1 <= H <= 64',
                   'F = 12': "pygat_amd dot_attention: F = 12: a head's width must be a power of two in 4..256; zero-padding the columns of q, k and "
                             'v to the next allowed F leaves the first F columns of the result unchanged (pass scale yourself: the default follows '
                             'the padded F)',
                   'F = 2': "pygat_amd dot_attention: F = 2: a head's width must be a power of two in 4..256; zero-padding the columns of q, k and v "
                            'to the next allowed F leaves the first F columns of the result unchanged (pass scale yourself: the default follows the '
                            'padded F)',
                   'F = 512': "pygat_amd dot_attention: F = 512: a head's width must be a power of two in 4..256; zero-padding the columns of q, k "
                              'and v to the next allowed F leaves the first F columns of the result unchanged (pass scale yourself: the default '
                              'follows the padded F)',
                   'H * F = 2048': 'pygat_amd dot_attention: H * F = 8 * 256 = 2048 floats per row: the limit is H * F <= 1024; zero-padding the '
                                   'columns of q, k and v to the next allowed F leaves the first F columns of the result unchanged (pass scale '
                                   'yourself: the default follows the padded F)'},
 'dot_attention.bias': {'no pattern': 'pygat_amd dot_attention: an EdgePattern expected (EdgePattern.from_indices, CSRGraph.edge_pattern)',
                        'another device': 'pygat_amd dot_attention: bias lives on cpu, the pattern on cuda:1',
                        'q no tensor': 'pygat_amd dot_attention: q must be a tensor on the GPU (there is no CPU path)',
                        'q on the cpu': 'pygat_amd dot_attention: q must be a tensor on the GPU (there is no CPU path)',
                        'q float64': 'pygat_amd dot_attention: q must be float32, not torch.float64',
                        'q torch.bfloat16': 'pygat_amd dot_attention: q must be float32, not torch.bfloat16',
                        'q one more dimension': 'pygat_amd dot_attention: q [n_rows, F] or [n_rows, H, F] expected, got (5, 2, 8, 1)',
                        'q of 3 heads': 'pygat_amd dot_attention: k (7, 2, 8) does not match q (5, 3, 8): the same number of heads and the same F '
                                        'expected',
                        'q of F = 4': 'pygat_amd dot_attention: k (7, 2, 8) does not match q (5, 2, 4): the same number of heads and the same F '
                                      'expected',
                        'q one more row': 'pygat_amd dot_attention: q has 6 rows but the pattern has 5 rows',
                        'k no tensor': 'pygat_amd dot_attention: k must be a tensor on the GPU (there is no CPU path)',
                        'k on the cpu': 'pygat_amd dot_attention: k must be a tensor on the GPU (there is no CPU path)',
                        'k float64': 'pygat_amd dot_attention: k must be float32, not torch.float64',
                        'k torch.bfloat16': 'pygat_amd dot_attention: k is torch.bfloat16 and v is torch.float32: the inference forward takes both k '
                                            'and v as bfloat16 tables (k.bfloat16(), v.bfloat16()); otherwise both are float32',
                        'k one more dimension': 'pygat_amd dot_attention: k (7, 2, 8, 1) does not match q (5, 2, 8): the same number of heads and '
                                                'the same F expected',
                        'k of 3 heads': 'pygat_amd dot_attention: k (7, 3, 8) does not match q (5, 2, 8): the same number of heads and the same F '
                                        'expected',
                        'k of F = 4': 'pygat_amd dot_attention: k (7, 2, 4) does not match q (5, 2, 8): the same number of heads and the same F '
                                      'expected',
                        'k one more row': 'pygat_amd dot_attention: k has 8 rows but the pattern has 7 columns',
                        'v no tensor': 'pygat_amd dot_attention: v must be a tensor on the GPU (there is no CPU path)',
                        'v on the cpu': 'pygat_amd dot_attention: v must be a tensor on the GPU (there is no CPU path)',
                        'v float64': 'pygat_amd dot_attention: v must be float32, not torch.float64',
                        'v torch.bfloat16': 'pygat_amd dot_attention: k is torch.float32 and v is torch.bfloat16: the inference forward takes both k '
                                            'and v as bfloat16 tables (k.bfloat16(), v.bfloat16()); otherwise both are float32',
                        'v one more dimension': 'pygat_amd dot_attention: v (7, 2, 8, 1) does not match q (5, 2, 8): the same number of heads and '
                                                'the same F expected',
                        'v of 3 heads': 'pygat_amd dot_attention: v (7, 3, 8) does not match q (5, 2, 8): the same number of heads and the same F '
                                        'expected',
                        'v of F = 4': 'pygat_amd dot_attention: v (7, 2, 4) does not match q (5, 2, 8): the same number of heads and the same F '
                                      'expected',
                        'v one more row': 'pygat_amd dot_attention: v has 8 rows but the pattern has 7 columns',
                        'bias no tensor': 'pygat_amd dot_attention: bias must be a tensor on the GPU (there is no CPU path)',
                        'bias on the cpu': 'pygat_amd dot_attention: bias must be a tensor on the GPU (there is no CPU path)',
                        'bias float64': 'pygat_amd dot_attention: bias must be float32, not torch.float64',
                        'bias torch.bfloat16': 'pygat_amd dot_attention: bias must be float32, not torch.bfloat16',
                        'bias one more dimension': 'pygat_amd dot_attention: bias [E, H] = [11, 2] or [E] = [11] expected for E = 11 entries and H = '
                                                   '2 heads, got (11, 2, 1)',
                        'bias of 3 heads': 'pygat_amd dot_attention: bias [E, H] = [11, 2] or [E] = [11] expected for E = 11 entries and H = 2 '
                                           'heads, got (11, 3)',
                        'bias one more row': 'pygat_amd dot_attention: bias [E, H] = [11, 2] or [E] = [11] expected for E = 11 entries and H = 2 '
                                             'heads, got (12, 2)',
                        'H = 65': 'pygat_amd dot_attention: H = 65 heads: the limits are 1 <= H <= 64',
                        'F = 12': "pygat_amd dot_attention: F = 12: a head's width must be a power of two in 4..256; zero-padding the columns of q, "
                                  'k and v to the next allowed F leaves the first F columns of the result unchanged (pass scale yourself: the '
                                  'default follows the padded F)',
                        'F = 2': "pygat_amd dot_attention: F = 2: a head's width must be a power of two in 4..256; zero-padding the columns of q, k "
                                 'and v to the next allowed F leaves the first F columns of the result unchanged (pass scale yourself: the default '
                                 'follows the padded F)',
                        'F = 512': "pygat_amd dot_attention: F = 512: a head's width must be a power of two in 4..256; zero-padding the columns of "
                                   'q, k and v to the next allowed F leaves the first F columns of the result unchanged (pass scale yourself: the '
                                   'default follows the padded F)',
                        'H * F = 2048': 'pygat_amd dot_attention: H * F = 8 * 256 = 2048 floats per row: the limit is H * F <= 1024; zero-padding '
                                        'the columns of q, k and v to the next allowed F leaves the first F columns of the result unchanged (pass '
                                        'scale yourself: the default follows the padded F)',
                        'bias [E, 1] beside heads': 'pygat_amd dot_attention: bias [E, H] = [11, 2] or [E] = [11] expected for E = 11 entries and H '
                                                    '= 2 heads, got (11, 1)',
                        'bias [E, H] without a head axis': 'pygat_amd dot_attention: bias [E] = [11] expected for E = 11 entries and H = 1 heads, '
                                                           'got (11, 2)'},
 'dot_attention.bf16': {'no pattern': 'pygat_amd dot_attention: an EdgePattern expected (EdgePattern.from_indices, CSRGraph.edge_pattern)',
                        'another device': 'pygat_amd dot_attention: bias lives on cpu, the pattern on cuda:1',
                        'q no tensor': 'pygat_amd dot_attention: q must be a tensor on the GPU (there is no CPU path)',
                        'q on the cpu': 'pygat_amd dot_attention: q must be a tensor on the GPU (there is no CPU path)',
                        'q float64': 'pygat_amd dot_attention: q must be float32, not torch.float64',
                        'q torch.bfloat16': 'pygat_amd dot_attention: q must be float32, not torch.bfloat16',
                        'q one more dimension': 'pygat_amd dot_attention: q [n_rows, F] or [n_rows, H, F] expected, got (5, 2, 8, 1)',
                        'q of 3 heads': 'pygat_amd dot_attention: k (7, 2, 8) does not match q (5, 3, 8): the same number of heads and the same F '
                                        'expected',
                        'q of F = 4': 'pygat_amd dot_attention: k (7, 2, 8) does not match q (5, 2, 4): the same number of heads and the same F '
                                      'expected',
                        'q one more row': 'pygat_amd dot_attention: q has 6 rows but the pattern has 5 rows',
                        'k no tensor': 'pygat_amd dot_attention: k is list and v is torch.bfloat16: the inference forward takes both k and v as '
                                       'bfloat16 tables (k.bfloat16(), v.bfloat16()); otherwise both are float32',
                        'k on the cpu': 'pygat_amd dot_attention: k must be a tensor on the GPU (there is no CPU path)',
                        'k float64': 'pygat_amd dot_attention: k is torch.float64 and v is torch.bfloat16: the inference forward takes both k and v '
                                     'as bfloat16 tables (k.bfloat16(), v.bfloat16()); otherwise both are float32',
                        'k torch.float32': 'pygat_amd dot_attention: k is torch.float32 and v is torch.bfloat16: the inference forward takes both k '
                                           'and v as bfloat16 tables (k.bfloat16(), v.bfloat16()); otherwise both are float32',
                        'k one more dimension': 'pygat_amd dot_attention: k (7, 2, 8, 1) does not match q (5, 2, 8): the same number of heads and '
                                                'the same F expected',
                        'k of 3 heads': 'pygat_amd dot_attention: k (7, 3, 8) does not match q (5, 2, 8): the same number of heads and the same F '
                                        'expected',
                        'k of F = 4': 'pygat_amd dot_attention: k (7, 2, 4) does not match q (5, 2, 8): the same number of heads and the same F '
                                      'expected',
                        'k one more row': 'pygat_amd dot_attention: k has 8 rows but the pattern has 7 columns',
                        'v no tensor': 'pygat_amd dot_attention: k is torch.bfloat16 and v is list: the inference forward takes both k and v as '
                                       'bfloat16 tables (k.bfloat16(), v.bfloat16()); otherwise both are float32',
                        'v on the cpu': 'pygat_amd dot_attention: v must be a tensor on the GPU (there is no CPU path)',
                        'v float64': 'pygat_amd dot_attention: k is torch.bfloat16 and v is torch.float64: the inference forward takes both k and v '
                                     'as bfloat16 tables (k.bfloat16(), v.bfloat16()); otherwise both are float32',
                        'v torch.float32': 'pygat_amd dot_attention: k is torch.bfloat16 and v is torch.float32: the inference forward takes both k '
                                           'and v as bfloat16 tables (k.bfloat16(), v.bfloat16()); otherwise both are float32',
                        'v one more dimension': 'pygat_amd dot_attention: v (7, 2, 8, 1) does not match q (5, 2, 8): the same number of heads and '
                                                'the same F expected',
                        'v of 3 heads': 'pygat_amd dot_attention: v (7, 3, 8) does not match q (5, 2, 8): the same number of heads and the same F '
                                        'expected',
                        'v of F = 4': 'pygat_amd dot_attention: v (7, 2, 4) does not match q (5, 2, 8): the same number of heads and the same F '
                                      'expected',
                        'v one more row': 'pygat_amd dot_attention: v has 8 rows but the pattern has 7 columns',
                        'bias no tensor': 'pygat_amd dot_attention: bias must be a tensor on the GPU (there is no CPU path)',
                        'bias on the cpu': 'pygat_amd dot_attention: bias must be a tensor on the GPU (there is no CPU path)',
                        'bias float64': 'pygat_amd dot_attention: bias must be float32, not torch.float64',
                        'bias torch.bfloat16': 'pygat_amd dot_attention: bias must be float32, not torch.bfloat16',
                        'bias one more dimension': 'pygat_amd dot_attention: bias [E, H] = [11, 2] or [E] = [11] expected for E = 11 entries and H = '
                                                   '2 heads, got (11, 2, 1)',
                        'bias of 3 heads': 'pygat_amd dot_attention: bias [E, H] = [11, 2] or [E] = [11] expected for E = 11 entries and H = 2 '
                                           'heads, got (11, 3)',
                        'bias one more row': 'pygat_amd dot_attention: bias [E, H] = [11, 2] or [E] = [11] expected for E = 11 entries and H = 2 '
                                             'heads, got (12, 2)',
                        'H = 65': 'pygat_amd dot_attention: H = 65 heads: the limits are 1 <= H <= 64',
                        'F = 12': "pygat_amd dot_attention: F = 12: a head's width must be a power of two in 4..256; zero-padding the columns of q, "
                                  'k and v to the next allowed F leaves the first F columns of the result unchanged (pass scale yourself: the '
                                  'default follows the padded F)',
                        'F = 2': "pygat_amd dot_attention: F = 2: a head's width must be a power of two in 4..256; zero-padding the columns of q, k "
                                 'and v to the next allowed F leaves the first F columns of the result unchanged (pass scale yourself: the default '
                                 'follows the padded F)',
                        'F = 512': "pygat_amd dot_attention: F = 512: a head's width must be a power of two in 4..256; zero-padding the columns of "
                                   'q, k and v to the next allowed F leaves the first F columns of the result unchanged (pass scale yourself: the '
                                   'default follows the padded F)',
                        'H * F = 2048': 'pygat_amd dot_attention: H * F = 8 * 256 = 2048 floats per row: the limit is H * F <= 1024; zero-padding '
                                        'the columns of q, k and v to the next allowed F leaves the first F columns of the result unchanged (pass '
                                        'scale yourself: the default follows the padded F)',
                        'bias [E, 1] beside heads': 'pygat_amd dot_attention: bias [E, H] = [11, 2] or [E] = [11] expected for E = 11 entries and H '
                                                    '= 2 heads, got (11, 1)',
                        'bias [E, H] without a head axis': 'pygat_amd dot_attention: bias [E] = [11] expected for E = 11 entries and H = 1 heads, '
                                                           'got (11, 2)',
                        'q requires grad': 'pygat_amd dot_attention: bfloat16 k and v are for inference (there is no backward through them): call it '
                                           'under torch.no_grad(), or pass float32 tables',
                        'k requires grad': 'pygat_amd dot_attention: bfloat16 k and v are for inference (there is no backward through them): call it '
                                           'under torch.no_grad(), or pass float32 tables',
                        'v requires grad': 'pygat_amd dot_attention: bfloat16 k and v are for inference (there is no backward through them): call it '
                                           'under torch.no_grad(), or pass float32 tables',
                        'bias requires grad': 'pygat_amd dot_attention: bfloat16 k and v are for inference (there is no backward through them): call '
                                              'it under torch.no_grad(), or pass float32 tables'},
 'dot_attention_dropout': {'no pattern': 'pygat_amd dot_attention_dropout: an EdgePattern expected (EdgePattern.from_indices, CSRGraph.edge_pattern)',
                           'another device': 'pygat_amd dot_attention_dropout: bias lives on cpu, the pattern on cuda:1',
                           'q no tensor': 'pygat_amd dot_attention_dropout: q must be a tensor on the GPU (there is no CPU path)',
                           'q on the cpu': 'pygat_amd dot_attention_dropout: q must be a tensor on the GPU (there is no CPU path)',
                           'q float64': 'pygat_amd dot_attention_dropout: q must be float32, not torch.float64',
                           'q torch.bfloat16': 'pygat_amd dot_attention_dropout: q must be float32, not torch.bfloat16',
                           'q one more dimension': 'pygat_amd dot_attention_dropout: q [n_rows, F] or [n_rows, H, F] expected, got (5, 2, 8, 1)',
                           'q of 3 heads': 'pygat_amd dot_attention_dropout: k (7, 2, 8) does not match q (5, 3, 8): the same number of heads and '
                                           'the same F expected',
                           'q of F = 4': 'pygat_amd dot_attention_dropout: k (7, 2, 8) does not match q (5, 2, 4): the same number of heads and the '
                                         'same F expected',
                           'q one more row': 'pygat_amd dot_attention_dropout: q has 6 rows but the pattern has 5 rows',
                           'k no tensor': 'pygat_amd dot_attention_dropout: k must be a tensor on the GPU (there is no CPU path)',
                           'k on the cpu': 'pygat_amd dot_attention_dropout: k must be a tensor on the GPU (there is no CPU path)',
                           'k float64': 'pygat_amd dot_attention_dropout: k must be float32, not torch.float64',
                           'k torch.bfloat16': 'pygat_amd dot_attention_dropout: k and v must be float32: there is no training path on bfloat16 '
                                               "tables (they are for dot_attention's inference forward)",
                           'k one more dimension': 'pygat_amd dot_attention_dropout: k (7, 2, 8, 1) does not match q (5, 2, 8): the same number of '
                                                   'heads and the same F expected',
                           'k of 3 heads': 'pygat_amd dot_attention_dropout: k (7, 3, 8) does not match q (5, 2, 8): the same number of heads and '
                                           'the same F expected',
                           'k of F = 4': 'pygat_amd dot_attention_dropout: k (7, 2, 4) does not match q (5, 2, 8): the same number of heads and the '
                                         'same F expected',
                           'k one more row': 'pygat_amd dot_attention_dropout: k has 8 rows but the pattern has 7 columns',
                           'v no tensor': 'pygat_amd dot_attention_dropout: v must be a tensor on the GPU (there is no CPU path)',
                           'v on the cpu': 'pygat_amd dot_attention_dropout: v must be a tensor on the GPU (there is no CPU path)',
                           'v float64': 'pygat_amd dot_attention_dropout: v must be float32, not torch.float64',
                           'v torch.bfloat16': 'pygat_amd dot_attention_dropout: k and v must be float32: there is no training path on bfloat16 '
                                               "tables (they are for dot_attention's inference forward)",
                           'v one more dimension': 'pygat_amd dot_attention_dropout: v (7, 2, 8, 1) does not match q (5, 2, 8): the same number of '
                                                   'heads and the same F expected',
                           'v of 3 heads': 'pygat_amd dot_attention_dropout: v (7, 3, 8) does not match q (5, 2, 8): the same number of heads and '
                                           'the same F expected',
                           'v of F = 4': 'pygat_amd dot_attention_dropout: v (7, 2, 4) does not match q (5, 2, 8): the same number of heads and the '
                                         'same F expected',
                           'v one more row': 'pygat_amd dot_attention_dropout: v has 8 rows but the pattern has 7 columns',
                           'bias no tensor': 'pygat_amd dot_attention_dropout: bias must be a tensor on the GPU (there is no CPU path)',
                           'bias on the cpu': 'pygat_amd dot_attention_dropout: bias must be a tensor on the GPU (there is no CPU path)',
                           'bias float64': 'pygat_amd dot_attention_dropout: bias must be float32, not torch.float64',
                           'bias torch.bfloat16': 'pygat_amd dot_attention_dropout: bias must be float32, not torch.bfloat16',
                           'bias one more dimension': 'pygat_amd dot_attention_dropout: bias [E, H] = [11, 2] or [E] = [11] expected for E = 11 '
                                                      'entries and H = 2 heads, got (11, 2, 1)',
                           'bias of 3 heads': 'pygat_amd dot_attention_dropout: bias [E, H] = [11, 2] or [E] = [11] expected for E = 11 entries and '
                                              'H = 2 heads, got (11, 3)',
                           'bias one more row': 'pygat_amd dot_attention_dropout: bias [E, H] = [11, 2] or [E] = [11] expected for E = 11 entries '
                                                'and H = 2 heads, got (12, 2)',
                           'H = 65': 'pygat_amd dot_attention_dropout: H = 65 heads: the limits are 1 <= H <= 64',
                           'F = 12': "pygat_amd dot_attention_dropout: F = 12: a head's width must be a power of two in 4..256; zero-padding the "
                                     'columns of q, k and v to the next allowed F leaves the first F columns of the result unchanged (pass scale '
                                     'yourself: the default follows the padded F)',
                           'F = 2': "pygat_amd dot_attention_dropout: F = 2: a head's width must be a power of two in 4..256; zero-padding the "
                                    'columns of q, k and v to the next allowed F leaves the first F columns of the result unchanged (pass scale '
                                    'yourself: the default follows the padded F)',
                           'F = 512': "pygat_amd dot_attention_dropout: F = 512: a head's width must be a power of two in 4..256; zero-padding the "
                                      'columns of q, k and v to the next allowed F leaves the first F columns of the result unchanged (pass scale '
                                      'yourself: the default follows the padded F)',
                           'H * F = 2048': 'pygat_amd dot_attention_dropout: H * F = 8 * 256 = 2048 floats per row: the limit is H * F <= 1024; '
                                           'zero-padding the columns of q, k and v to the next allowed F leaves the first F columns of the result '
                                           'unchanged (pass scale yourself: the default follows the padded F)',
                           'bias [E, 1] beside heads': 'pygat_amd dot_attention_dropout: bias [E, H] = [11, 2] or [E] = [11] expected for E = 11 '
                                                       'entries and H = 2 heads, got (11, 1)',
                           'bias [E, H] without a head axis': 'pygat_amd dot_attention_dropout: bias [E] = [11] expected for E = 11 entries and H = '
                                                              '1 heads, got (11, 2)',
                           'p -0.1': 'pygat_amd dot_attention_dropout: p = -0.1: a dropout probability in [0, 1] expected',
                           'p 1.5': 'pygat_amd dot_attention_dropout: p = 1.5: a dropout probability in [0, 1] expected',
                           'p True': 'pygat_amd dot_attention_dropout: p = True: a dropout probability in [0, 1] expected',
                           'p nan': 'pygat_amd dot_attention_dropout: p = nan: a dropout probability in [0, 1] expected',
                           'seed dtype': "pygat_amd dot_attention_dropout: seed must be an int64 tensor of shape [1] on the pattern's device cpu "
                                         '(the kernels read it there, so a captured graph replays with the value it finds), got torch.int32 (1,) on '
                                         'cpu',
                           'seed shape': "pygat_amd dot_attention_dropout: seed must be an int64 tensor of shape [1] on the pattern's device cpu "
                                         '(the kernels read it there, so a captured graph replays with the value it finds), got torch.int64 (2,) on '
                                         'cpu',
                           'seed no tensor': "pygat_amd dot_attention_dropout: seed must be an int64 tensor of shape [1] on the pattern's device cpu "
                                             '(the kernels read it there, so a captured graph replays with the value it finds), got int'},
 'dot_attention_edge': {'no pattern': 'pygat_amd dot_attention_edge: an EdgePattern expected (EdgePattern.from_indices, CSRGraph.edge_pattern)',
                        'another device': 'pygat_amd dot_attention_edge: e lives on cpu, the pattern on cuda:1; e [E, H, F] (or [E, F] without a '
                                          "head axis), a row per entry at the caller's entry index, expected",
                        'q no tensor': 'pygat_amd dot_attention_edge: q must be a tensor on the GPU (there is no CPU path)',
                        'q on the cpu': 'pygat_amd dot_attention_edge: q must be a tensor on the GPU (there is no CPU path)',
                        'q float64': 'pygat_amd dot_attention_edge: q must be float32, not torch.float64',
                        'q torch.bfloat16': 'pygat_amd dot_attention_edge: q must be float32, not torch.bfloat16',
                        'q one more dimension': 'pygat_amd dot_attention_edge: q [n_rows, F] or [n_rows, H, F] expected, got (5, 2, 8, 1)',
                        'q of 3 heads': 'pygat_amd dot_attention_edge: k (7, 2, 8) does not match q (5, 3, 8): the same number of heads and the same '
                                        'F expected',
                        'q of F = 4': 'pygat_amd dot_attention_edge: k (7, 2, 8) does not match q (5, 2, 4): the same number of heads and the same F '
                                      'expected',
                        'q one more row': 'pygat_amd dot_attention_edge: q has 6 rows but the pattern has 5 rows',
                        'k no tensor': 'pygat_amd dot_attention_edge: k must be a tensor on the GPU (there is no CPU path)',
                        'k on the cpu': 'pygat_amd dot_attention_edge: k must be a tensor on the GPU (there is no CPU path)',
                        'k float64': 'pygat_amd dot_attention_edge: k must be float32, not torch.float64',
                        'k torch.bfloat16': "pygat_amd dot_attention_edge: k, v and e must be float32: bfloat16 tables are for dot_attention's "
                                            'inference forward',
                        'k one more dimension': 'pygat_amd dot_attention_edge: k (7, 2, 8, 1) does not match q (5, 2, 8): the same number of heads '
                                                'and the same F expected',
                        'k of 3 heads': 'pygat_amd dot_attention_edge: k (7, 3, 8) does not match q (5, 2, 8): the same number of heads and the same '
                                        'F expected',
                        'k of F = 4': 'pygat_amd dot_attention_edge: k (7, 2, 4) does not match q (5, 2, 8): the same number of heads and the same F '
                                      'expected',
                        'k one more row': 'pygat_amd dot_attention_edge: k has 8 rows but the pattern has 7 columns',
                        'v no tensor': 'pygat_amd dot_attention_edge: v must be a tensor on the GPU (there is no CPU path)',
                        'v on the cpu': 'pygat_amd dot_attention_edge: v must be a tensor on the GPU (there is no CPU path)',
                        'v float64': 'pygat_amd dot_attention_edge: v must be float32, not torch.float64',
                        'v torch.bfloat16': "pygat_amd dot_attention_edge: k, v and e must be float32: bfloat16 tables are for dot_attention's "
                                            'inference forward',
                        'v one more dimension': 'pygat_amd dot_attention_edge: v (7, 2, 8, 1) does not match q (5, 2, 8): the same number of heads '
                                                'and the same F expected',
                        'v of 3 heads': 'pygat_amd dot_attention_edge: v (7, 3, 8) does not match q (5, 2, 8): the same number of heads and the same '
                                        'F expected',
                        'v of F = 4': 'pygat_amd dot_attention_edge: v (7, 2, 4) does not match q (5, 2, 8): the same number of heads and the same F '
                                      'expected',
                        'v one more row': 'pygat_amd dot_attention_edge: v has 8 rows but the pattern has 7 columns',
                        'e no tensor': 'pygat_amd dot_attention_edge: e must be a tensor on the GPU (there is no CPU path); e [E, H, F] (or [E, F] '
                                       "without a head axis), a row per entry at the caller's entry index, expected",
                        'e on the cpu': 'pygat_amd dot_attention_edge: e must be a tensor on the GPU (there is no CPU path); e [E, H, F] (or [E, F] '
                                        "without a head axis), a row per entry at the caller's entry index, expected",
                        'e float64': 'pygat_amd dot_attention_edge: e must be float32, not torch.float64; e [E, H, F] (or [E, F] without a head '
                                     "axis), a row per entry at the caller's entry index, expected",
                        'e torch.bfloat16': "pygat_amd dot_attention_edge: k, v and e must be float32: bfloat16 tables are for dot_attention's "
                                            'inference forward',
                        'e one more dimension': 'pygat_amd dot_attention_edge: e [11, 2, 8] expected for E = 11 entries and q (5, 2, 8) -- (E,) + '
                                                'q.shape[1:], a row per entry -- got (11, 2, 8, 1)',
                        'e of 3 heads': 'pygat_amd dot_attention_edge: e [11, 2, 8] expected for E = 11 entries and q (5, 2, 8) -- (E,) + '
                                        'q.shape[1:], a row per entry -- got (11, 3, 8)',
                        'e of F = 4': 'pygat_amd dot_attention_edge: e [11, 2, 8] expected for E = 11 entries and q (5, 2, 8) -- (E,) + q.shape[1:], '
                                      'a row per entry -- got (11, 2, 4)',
                        'e one more row': 'pygat_amd dot_attention_edge: e [11, 2, 8] expected for E = 11 entries and q (5, 2, 8) -- (E,) + '
                                          'q.shape[1:], a row per entry -- got (12, 2, 8)',
                        'bias no tensor': 'pygat_amd dot_attention_edge: bias must be a tensor on the GPU (there is no CPU path)',
                        'bias on the cpu': 'pygat_amd dot_attention_edge: bias must be a tensor on the GPU (there is no CPU path)',
                        'bias float64': 'pygat_amd dot_attention_edge: bias must be float32, not torch.float64',
                        'bias torch.bfloat16': 'pygat_amd dot_attention_edge: bias must be float32, not torch.bfloat16',
                        'bias one more dimension': 'pygat_amd dot_attention_edge: bias [E, H] = [11, 2] or [E] = [11] expected for E = 11 entries '
                                                   'and H = 2 heads, got (11, 2, 1)',
                        'bias of 3 heads': 'pygat_amd dot_attention_edge: bias [E, H] = [11, 2] or [E] = [11] expected for E = 11 entries and H = 2 '
                                           'heads, got (11, 3)',
                        'bias one more row': 'pygat_amd dot_attention_edge: bias [E, H] = [11, 2] or [E] = [11] expected for E = 11 entries and H = '
                                             '2 heads, got (12, 2)',
                        'H = 65': 'pygat_amd dot_attention_edge: H = 65 heads: the limits are 1 <= H <= 64',
                        'F = 12': "pygat_amd dot_attention_edge: F = 12: a head's width must be a power of two in 4..256; zero-padding the columns "
                                  'of q, k and v to the next allowed F leaves the first F columns of the result unchanged (pass scale yourself: the '
                                  'default follows the padded F)',
                        'F = 2': "pygat_amd dot_attention_edge: F = 2: a head's width must be a power of two in 4..256; zero-padding the columns of "
                                 'q, k and v to the next allowed F leaves the first F columns of the result unchanged (pass scale yourself: the '
                                 'default follows the padded F)',
                        'F = 512': "pygat_amd dot_attention_edge: F = 512: a head's width must be a power of two in 4..256; zero-padding the columns "
                                   'of q, k and v to the next allowed F leaves the first F columns of the result unchanged (pass scale yourself: the '
                                   'default follows the padded F)',
                        'H * F = 2048': 'pygat_amd dot_attention_edge: H * F = 8 * 256 = 2048 floats per row: the limit is H * F <= 1024; '
                                        'zero-padding the columns of q, k and v to the next allowed F leaves the first F columns of the result '
                                        'unchanged (pass scale yourself: the default follows the padded F)',
                        'bias [E, 1] beside heads': 'pygat_amd dot_attention_edge: bias [E, H] = [11, 2] or [E] = [11] expected for E = 11 entries '
                                                    'and H = 2 heads, got (11, 1)',
                        'bias [E, H] without a head axis': 'pygat_amd dot_attention_edge: bias [E] = [11] expected for E = 11 entries and H = 1 '
                                                           'heads, got (11, 2)'},
 'additive_attention': {'no pattern': 'pygat_amd additive_attention: an EdgePattern expected (EdgePattern.from_indices, CSRGraph.edge_pattern)',
                        'another device': 'pygat_amd additive_attention: edge_logit lives on cpu, the pattern on cuda:1',
                        's_dst no tensor': 'pygat_amd additive_attention: s_dst must be a tensor on the GPU (there is no CPU path)',
                        's_dst on the cpu': 'pygat_amd additive_attention: s_dst must be a tensor on the GPU (there is no CPU path)',
                        's_dst float64': 'pygat_amd additive_attention: s_dst must be float32, not torch.float64',
                        's_dst torch.bfloat16': 'pygat_amd additive_attention: s_dst must be float32, not torch.bfloat16',
                        's_dst one more dimension': 'pygat_amd additive_attention: s_dst [n_rows] or [n_rows, H] expected, got (5, 2, 1)',
                        's_dst of 3 heads': 'pygat_amd additive_attention: s_src (7, 2) does not match s_dst (5, 3): the same number of heads '
                                            'expected',
                        's_dst one more row': 'pygat_amd additive_attention: s_dst has 6 rows but the pattern has 5 rows',
                        's_src no tensor': 'pygat_amd additive_attention: s_src must be a tensor on the GPU (there is no CPU path)',
                        's_src on the cpu': 'pygat_amd additive_attention: s_src must be a tensor on the GPU (there is no CPU path)',
                        's_src float64': 'pygat_amd additive_attention: s_src must be float32, not torch.float64',
                        's_src torch.bfloat16': 'pygat_amd additive_attention: s_src must be float32, not torch.bfloat16',
                        's_src one more dimension': 'pygat_amd additive_attention: s_src (7, 2, 1) does not match s_dst (5, 2): the same number of '
                                                    'heads expected',
                        's_src of 3 heads': 'pygat_amd additive_attention: s_src (7, 3) does not match s_dst (5, 2): the same number of heads '
                                            'expected',
                        's_src one more row': 'pygat_amd additive_attention: s_src has 8 rows but the pattern has 7 columns',
                        'v no tensor': 'pygat_amd additive_attention: v must be a tensor on the GPU (there is no CPU path)',
                        'v on the cpu': 'pygat_amd additive_attention: v must be a tensor on the GPU (there is no CPU path)',
                        'v float64': 'pygat_amd additive_attention: v must be float32, not torch.float64',
                        'v torch.bfloat16': 'pygat_amd additive_attention: v must be float32, not torch.bfloat16',
                        'v one more dimension': 'pygat_amd additive_attention: v (7, 2, 8, 1) does not match s_dst (5, 2): v [n_cols, F] with s_dst '
                                                '[n_rows], or v [n_cols, H, F] with s_dst [n_rows, H] and the same number of heads, expected',
                        'v of 3 heads': 'pygat_amd additive_attention: v (7, 3, 8) does not match s_dst (5, 2): v [n_cols, F] with s_dst [n_rows], '
                                        'or v [n_cols, H, F] with s_dst [n_rows, H] and the same number of heads, expected',
                        'v one more row': 'pygat_amd additive_attention: v has 8 rows but the pattern has 7 columns',
                        'edge_logit no tensor': 'pygat_amd additive_attention: edge_logit must be a tensor on the GPU (there is no CPU path)',
                        'edge_logit on the cpu': 'pygat_amd additive_attention: edge_logit must be a tensor on the GPU (there is no CPU path)',
                        'edge_logit float64': 'pygat_amd additive_attention: edge_logit must be float32, not torch.float64',
                        'edge_logit torch.bfloat16': 'pygat_amd additive_attention: edge_logit must be float32, not torch.bfloat16',
                        'edge_logit one more dimension': 'pygat_amd additive_attention: edge_logit [E, H] = [11, 2] or [E] = [11] expected for E = '
                                                         '11 entries and H = 2 heads, got (11, 2, 1)',
                        'edge_logit of 3 heads': 'pygat_amd additive_attention: edge_logit [E, H] = [11, 2] or [E] = [11] expected for E = 11 '
                                                 'entries and H = 2 heads, got (11, 3)',
                        'edge_logit one more row': 'pygat_amd additive_attention: edge_logit [E, H] = [11, 2] or [E] = [11] expected for E = 11 '
                                                   'entries and H = 2 heads, got (12, 2)',
                        'H = 65': 'pygat_amd additive_attention: H = 65 heads: the limits are 1 <= H <= 64',
                        'F = 12': "pygat_amd additive_attention: F = 12: a head's width must be a power of two in 4..256; zero-padding the columns "
                                  'of v to the next allowed F leaves the first F columns of the result unchanged (no scale depends on F)',
                        'F = 2': "pygat_amd additive_attention: F = 2: a head's width must be a power of two in 4..256; zero-padding the columns of "
                                 'v to the next allowed F leaves the first F columns of the result unchanged (no scale depends on F)',
                        'F = 512': "pygat_amd additive_attention: F = 512: a head's width must be a power of two in 4..256; zero-padding the columns "
                                   'of v to the next allowed F leaves the first F columns of the result unchanged (no scale depends on F)',
                        'H * F = 2048': 'pygat_amd additive_attention: H * F = 8 * 256 = 2048 floats per row: the limit is H * F <= 1024; '
                                        'zero-padding the columns of v to the next allowed F leaves the first F columns of the result unchanged (no '
                                        'scale depends on F)',
                        'edge_logit [E, 1] beside heads': 'pygat_amd additive_attention: edge_logit [E, H] = [11, 2] or [E] = [11] expected for E = '
                                                          '11 entries and H = 2 heads, got (11, 1)',
                        'edge_logit [E, H] without a head axis': 'pygat_amd additive_attention: edge_logit [E] = [11] expected for E = 11 entries '
                                                                 'and H = 1 heads, got (11, 2)',
                        'negative_slope True': 'pygat_amd additive_attention: negative_slope = True: a finite float expected',
                        'negative_slope inf': 'pygat_amd additive_attention: negative_slope = inf: a finite float expected'},
 'additive_attention_dropout': {'no pattern': 'pygat_amd additive_attention_dropout: an EdgePattern expected (EdgePattern.from_indices, '
                                              'CSRGraph.edge_pattern)',
                                'another device': 'pygat_amd additive_attention_dropout: edge_logit lives on cpu, the pattern on cuda:1',
                                's_dst no tensor': 'pygat_amd additive_attention_dropout: s_dst must be a tensor on the GPU (there is no CPU path)',
                                's_dst on the cpu': 'pygat_amd additive_attention_dropout: s_dst must be a tensor on the GPU (there is no CPU path)',
                                's_dst float64': 'pygat_amd additive_attention_dropout: s_dst must be float32, not torch.float64',
                                's_dst torch.bfloat16': 'pygat_amd additive_attention_dropout: s_dst, s_src, v and edge_logit must be float32: there '
                                                        'is no training path on bfloat16 tensors',
                                's_dst one more dimension': 'pygat_amd additive_attention_dropout: s_dst [n_rows] or [n_rows, H] expected, got (5, '
                                                            '2, 1)',
                                's_dst of 3 heads': 'pygat_amd additive_attention_dropout: s_src (7, 2) does not match s_dst (5, 3): the same number '
                                                    'of heads expected',
                                's_dst one more row': 'pygat_amd additive_attention_dropout: s_dst has 6 rows but the pattern has 5 rows',
                                's_src no tensor': 'pygat_amd additive_attention_dropout: s_src must be a tensor on the GPU (there is no CPU path)',
                                's_src on the cpu': 'pygat_amd additive_attention_dropout: s_src must be a tensor on the GPU (there is no CPU path)',
                                's_src float64': 'pygat_amd additive_attention_dropout: s_src must be float32, not torch.float64',
                                's_src torch.bfloat16': 'pygat_amd additive_attention_dropout: s_dst, s_src, v and edge_logit must be float32: there '
                                                        'is no training path on bfloat16 tensors',
                                's_src one more dimension': 'pygat_amd additive_attention_dropout: s_src (7, 2, 1) does not match s_dst (5, 2): the '
                                                            'same number of heads expected',
                                's_src of 3 heads': 'pygat_amd additive_attention_dropout: s_src (7, 3) does not match s_dst (5, 2): the same number '
                                                    'of heads expected',
                                's_src one more row': 'pygat_amd additive_attention_dropout: s_src has 8 rows but the pattern has 7 columns',
                                'v no tensor': 'pygat_amd additive_attention_dropout: v must be a tensor on the GPU (there is no CPU path)',
                                'v on the cpu': 'pygat_amd additive_attention_dropout: v must be a tensor on the GPU (there is no CPU path)',
                                'v float64': 'pygat_amd additive_attention_dropout: v must be float32, not torch.float64',
                                'v torch.bfloat16': 'pygat_amd additive_attention_dropout: s_dst, s_src, v and edge_logit must be float32: there is '
                                                    'no training path on bfloat16 tensors',
                                'v one more dimension': 'pygat_amd additive_attention_dropout: v (7, 2, 8, 1) does not match s_dst (5, 2): v '
                                                        '[n_cols, F] with s_dst [n_rows], or v [n_cols, H, F] with s_dst [n_rows, H] and the same '
                                                        'number of heads, expected',
                                'v of 3 heads': 'pygat_amd additive_attention_dropout: v (7, 3, 8) does not match s_dst (5, 2): v [n_cols, F] with '
                                                's_dst [n_rows], or v [n_cols, H, F] with s_dst [n_rows, H] and the same number of heads, expected',
                                'v one more row': 'pygat_amd additive_attention_dropout: v has 8 rows but the pattern has 7 columns',
                                'edge_logit no tensor': 'pygat_amd additive_attention_dropout: edge_logit must be a tensor on the GPU (there is no '
                                                        'CPU path)',
                                'edge_logit on the cpu': 'pygat_amd additive_attention_dropout: edge_logit must be a tensor on the GPU (there is no '
                                                         'CPU path)',
                                'edge_logit float64': 'pygat_amd additive_attention_dropout: edge_logit must be float32, not torch.float64',
                                'edge_logit torch.bfloat16': 'pygat_amd additive_attention_dropout: s_dst, s_src, v and edge_logit must be float32: '
                                                             'there is no training path on bfloat16 tensors',
                                'edge_logit one more dimension': 'pygat_amd additive_attention_dropout: edge_logit [E, H] = [11, 2] or [E] = [11] '
                                                                 'expected for E = 11 entries and H = 2 heads, got (11, 2, 1)',
                                'edge_logit of 3 heads': 'pygat_amd additive_attention_dropout: edge_logit [E, H] = [11, 2] or [E] = [11] expected '
                                                         'for E = 11 entries and H = 2 heads, got (11, 3)',
                                'edge_logit one more row': 'pygat_amd additive_attention_dropout: edge_logit [E, H] = [11, 2] or [E] = [11] expected '
                                                           'for E = 11 entries and H = 2 heads, got (12, 2)',
                                'H = 65': 'pygat_amd additive_attention_dropout: H = 65 heads: the limits are 1 <= H <= 64',
                                'F = 12': "pygat_amd additive_attention_dropout: F = 12: a head's width must be a power of two in 4..256; "
                                          'zero-padding the columns of v to the next allowed F leaves the first F columns of the result unchanged '
                                          '(no scale depends on F)',
                                'F = 2': "pygat_amd additive_attention_dropout: F = 2: a head's width must be a power of two in 4..256; zero-padding "
                                         'the columns of v to the next allowed F leaves the first F columns of the result unchanged (no scale '
                                         'depends on F)',
                                'F = 512': "pygat_amd additive_attention_dropout: F = 512: a head's width must be a power of two in 4..256; "
                                           'zero-padding the columns of v to the next allowed F leaves the first F columns of the result unchanged '
                                           '(no scale depends on F)',
                                'H * F = 2048': 'pygat_amd additive_attention_dropout: H * F = 8 * 256 = 2048 floats per row: the limit is H * F <= '
                                                '1024; zero-padding the columns of v to the next allowed F leaves the first F columns of the result '
                                                'unchanged (no scale depends on F)',
                                'edge_logit [E, 1] beside heads': 'pygat_amd additive_attention_dropout: edge_logit [E, H] = [11, 2] or [E] = [11] '
                                                                  'expected for E = 11 entries and H = 2 heads, got (11, 1)',
                                'edge_logit [E, H] without a head axis': 'pygat_amd additive_attention_dropout: edge_logit [E] = [11] expected for E '
                                                                         '= 11 entries and H = 1 heads, got (11, 2)',
                                'p -0.1': 'pygat_amd additive_attention_dropout: p = -0.1: a dropout probability in [0, 1] expected',
                                'p 1.5': 'pygat_amd additive_attention_dropout: p = 1.5: a dropout probability in [0, 1] expected',
                                'p True': 'pygat_amd additive_attention_dropout: p = True: a dropout probability in [0, 1] expected',
                                'p nan': 'pygat_amd additive_attention_dropout: p = nan: a dropout probability in [0, 1] expected',
                                'seed dtype': "pygat_amd additive_attention_dropout: seed must be an int64 tensor of shape [1] on the pattern's "
                                              'device cpu (the kernels read it there, so a captured graph replays with the value it finds), got '
                                              'torch.int32 (1,) on cpu',
                                'seed shape': "pygat_amd additive_attention_dropout: seed must be an int64 tensor of shape [1] on the pattern's "
                                              'device cpu (the kernels read it there, so a captured graph replays with the value it finds), got '
                                              'torch.int64 (2,) on cpu',
                                'seed no tensor': "pygat_amd additive_attention_dropout: seed must be an int64 tensor of shape [1] on the pattern's "
                                                  'device cpu (the kernels read it there, so a captured graph replays with the value it finds), got '
                                                  'int',
                                'negative_slope True': 'pygat_amd additive_attention_dropout: negative_slope = True: a finite float expected',
                                'negative_slope inf': 'pygat_amd additive_attention_dropout: negative_slope = inf: a finite float expected'},
 'additive_attention_bf16': {'no pattern': 'pygat_amd additive_attention_bf16: an EdgePattern expected (EdgePattern.from_indices, '
                                           'CSRGraph.edge_pattern)',
                             'another device': 'pygat_amd additive_attention_bf16: edge_logit lives on cpu, the pattern on cuda:1',
                             's_dst no tensor': 'pygat_amd additive_attention_bf16: s_dst must be a tensor on the GPU (there is no CPU path)',
                             's_dst on the cpu': 'pygat_amd additive_attention_bf16: s_dst must be a tensor on the GPU (there is no CPU path)',
                             's_dst float64': 'pygat_amd additive_attention_bf16: s_dst must be torch.float32, not torch.float64: it is float32 in '
                                              'this op: only the row tables of H * F values are bfloat16',
                             's_dst torch.bfloat16': 'pygat_amd additive_attention_bf16: s_dst must be torch.float32, not torch.bfloat16: it is '
                                                     'float32 in this op: only the row tables of H * F values are bfloat16',
                             's_dst one more dimension': 'pygat_amd additive_attention_bf16: s_dst [n_rows] or [n_rows, H] expected, got (5, 2, 1)',
                             's_dst of 3 heads': 'pygat_amd additive_attention_bf16: s_src (7, 2) does not match s_dst (5, 3): the same number of '
                                                 'heads expected',
                             's_dst one more row': 'pygat_amd additive_attention_bf16: s_dst has 6 rows but the pattern has 5 rows',
                             's_src no tensor': 'pygat_amd additive_attention_bf16: s_src must be a tensor on the GPU (there is no CPU path)',
                             's_src on the cpu': 'pygat_amd additive_attention_bf16: s_src must be a tensor on the GPU (there is no CPU path)',
                             's_src float64': 'pygat_amd additive_attention_bf16: s_src must be torch.float32, not torch.float64: it is float32 in '
                                              'this op: only the row tables of H * F values are bfloat16',
                             's_src torch.bfloat16': 'pygat_amd additive_attention_bf16: s_src must be torch.float32, not torch.bfloat16: it is '
                                                     'float32 in this op: only the row tables of H * F values are bfloat16',
                             's_src one more dimension': 'pygat_amd additive_attention_bf16: s_src (7, 2, 1) does not match s_dst (5, 2): the same '
                                                         'number of heads expected',
                             's_src of 3 heads': 'pygat_amd additive_attention_bf16: s_src (7, 3) does not match s_dst (5, 2): the same number of '
                                                 'heads expected',
                             's_src one more row': 'pygat_amd additive_attention_bf16: s_src has 8 rows but the pattern has 7 columns',
                             'v16 no tensor': 'pygat_amd additive_attention_bf16: v16 must be a tensor on the GPU (there is no CPU path)',
                             'v16 on the cpu': 'pygat_amd additive_attention_bf16: v16 must be a tensor on the GPU (there is no CPU path)',
                             'v16 float64': 'pygat_amd additive_attention_bf16: v16 must be torch.bfloat16, not torch.float64: it is a bfloat16 '
                                            'table of this op (make it once: t.bfloat16())',
                             'v16 torch.float32': 'pygat_amd additive_attention_bf16: v16 must be torch.bfloat16, not torch.float32: it is a '
                                                  'bfloat16 table of this op (make it once: t.bfloat16())',
                             'v16 one more dimension': 'pygat_amd additive_attention_bf16: v16 (7, 2, 8, 1) does not match s_dst (5, 2): v16 '
                                                       '[n_cols, F] with s_dst [n_rows], or v16 [n_cols, H, F] with s_dst [n_rows, H] and the same '
                                                       'number of heads, expected',
                             'v16 of 3 heads': 'pygat_amd additive_attention_bf16: v16 (7, 3, 8) does not match s_dst (5, 2): v16 [n_cols, F] with '
                                               's_dst [n_rows], or v16 [n_cols, H, F] with s_dst [n_rows, H] and the same number of heads, expected',
                             'v16 one more row': 'pygat_amd additive_attention_bf16: v16 has 8 rows but the pattern has 7 columns',
                             'edge_logit no tensor': 'pygat_amd additive_attention_bf16: edge_logit must be a tensor on the GPU (there is no CPU '
                                                     'path)',
                             'edge_logit on the cpu': 'pygat_amd additive_attention_bf16: edge_logit must be a tensor on the GPU (there is no CPU '
                                                      'path)',
                             'edge_logit float64': 'pygat_amd additive_attention_bf16: edge_logit must be torch.float32, not torch.float64: it is '
                                                   'float32 in this op: only the row tables of H * F values are bfloat16',
                             'edge_logit torch.bfloat16': 'pygat_amd additive_attention_bf16: edge_logit must be torch.float32, not torch.bfloat16: '
                                                          'it is float32 in this op: only the row tables of H * F values are bfloat16',
                             'edge_logit one more dimension': 'pygat_amd additive_attention_bf16: edge_logit [E, H] = [11, 2] or [E] = [11] expected '
                                                              'for E = 11 entries and H = 2 heads, got (11, 2, 1)',
                             'edge_logit of 3 heads': 'pygat_amd additive_attention_bf16: edge_logit [E, H] = [11, 2] or [E] = [11] expected for E = '
                                                      '11 entries and H = 2 heads, got (11, 3)',
                             'edge_logit one more row': 'pygat_amd additive_attention_bf16: edge_logit [E, H] = [11, 2] or [E] = [11] expected for E '
                                                        '= 11 entries and H = 2 heads, got (12, 2)',
                             'H = 65': 'pygat_amd additive_attention_bf16: H = 65 heads: the limits are 1 <= H <= 64',
                             'F = 12': "pygat_amd additive_attention_bf16: F = 12: a head's width must be a power of two in 4..256; zero-padding the "
                                       'columns of v to the next allowed F leaves the first F columns of the result unchanged (no scale depends on '
                                       'F)',
                             'F = 2': "pygat_amd additive_attention_bf16: F = 2: a head's width must be a power of two in 4..256; zero-padding the "
                                      'columns of v to the next allowed F leaves the first F columns of the result unchanged (no scale depends on F)',
                             'F = 512': "pygat_amd additive_attention_bf16: F = 512: a head's width must be a power of two in 4..256; zero-padding "
                                        'the columns of v to the next allowed F leaves the first F columns of the result unchanged (no scale depends '
                                        'on F)',
                             'H * F = 2048': 'pygat_amd additive_attention_bf16: H * F = 8 * 256 = 2048 floats per row: the limit is H * F <= 1024; '
                                             'zero-padding the columns of v to the next allowed F leaves the first F columns of the result unchanged '
                                             '(no scale depends on F)',
                             'edge_logit [E, 1] beside heads': 'pygat_amd additive_attention_bf16: edge_logit [E, H] = [11, 2] or [E] = [11] '
                                                               'expected for E = 11 entries and H = 2 heads, got (11, 1)',
                             'edge_logit [E, H] without a head axis': 'pygat_amd additive_attention_bf16: edge_logit [E] = [11] expected for E = 11 '
                                                                      'entries and H = 1 heads, got (11, 2)',
                             'negative_slope True': 'pygat_amd additive_attention_bf16: negative_slope = True: a finite float expected',
                             'negative_slope inf': 'pygat_amd additive_attention_bf16: negative_slope = inf: a finite float expected',
                             's_dst requires grad': 'pygat_amd additive_attention_bf16: bfloat16 tables are for inference (there is no backward '
                                                    'through this op) and an argument requires grad: call it under torch.no_grad(), or use '
                                                    'additive_attention on float32 tables',
                             's_src requires grad': 'pygat_amd additive_attention_bf16: bfloat16 tables are for inference (there is no backward '
                                                    'through this op) and an argument requires grad: call it under torch.no_grad(), or use '
                                                    'additive_attention on float32 tables',
                             'v16 requires grad': 'pygat_amd additive_attention_bf16: bfloat16 tables are for inference (there is no backward '
                                                  'through this op) and an argument requires grad: call it under torch.no_grad(), or use '
                                                  'additive_attention on float32 tables',
                             'edge_logit requires grad': 'pygat_amd additive_attention_bf16: bfloat16 tables are for inference (there is no backward '
                                                         'through this op) and an argument requires grad: call it under torch.no_grad(), or use '
                                                         'additive_attention on float32 tables'},
 'gatv2_attention': {'no pattern': 'pygat_amd gatv2_attention: an EdgePattern expected (EdgePattern.from_indices, CSRGraph.edge_pattern)',
                     'another device': 'pygat_amd gatv2_attention: x_dst lives on cpu, the pattern on cuda:1',
                     'x_dst no tensor': 'pygat_amd gatv2_attention: x_dst must be a tensor on the GPU (there is no CPU path)',
                     'x_dst on the cpu': 'pygat_amd gatv2_attention: x_dst must be a tensor on the GPU (there is no CPU path)',
                     'x_dst float64': 'pygat_amd gatv2_attention: x_dst must be float32, not torch.float64',
                     'x_dst torch.bfloat16': 'pygat_amd gatv2_attention: x_dst must be float32, not torch.bfloat16',
                     'x_dst one more dimension': 'pygat_amd gatv2_attention: x_dst [n_rows, F] or [n_rows, H, F] expected, got (5, 2, 8, 1)',
                     'x_dst of 3 heads': 'pygat_amd gatv2_attention: x_src (7, 2, 8) does not match x_dst (5, 3, 8): the same number of heads and '
                                         'the same width expected',
                     'x_dst of F = 4': 'pygat_amd gatv2_attention: x_src (7, 2, 8) does not match x_dst (5, 2, 4): the same number of heads and the '
                                       'same width expected',
                     'x_dst one more row': 'pygat_amd gatv2_attention: x_dst has 6 rows but the pattern has 5 rows',
                     'a no tensor': 'pygat_amd gatv2_attention: a must be a tensor on the GPU (there is no CPU path)',
                     'a on the cpu': 'pygat_amd gatv2_attention: a must be a tensor on the GPU (there is no CPU path)',
                     'a float64': 'pygat_amd gatv2_attention: a must be float32, not torch.float64',
                     'a torch.bfloat16': 'pygat_amd gatv2_attention: a must be float32, not torch.bfloat16',
                     'a one more dimension': 'pygat_amd gatv2_attention: a (2, 8, 1) does not match x_dst (5, 2, 8): a [F] with x_dst [n_rows, F], '
                                             'or a [H, F] with x_dst [n_rows, H, F], expected',
                     'a of 3 heads': 'pygat_amd gatv2_attention: a (3, 8) does not match x_dst (5, 2, 8): a [F] with x_dst [n_rows, F], or a [H, F] '
                                     'with x_dst [n_rows, H, F], expected',
                     'a of F = 4': 'pygat_amd gatv2_attention: a (2, 4) does not match x_dst (5, 2, 8): a [F] with x_dst [n_rows, F], or a [H, F] '
                                   'with x_dst [n_rows, H, F], expected',
                     'x_src no tensor': 'pygat_amd gatv2_attention: x_src must be a tensor on the GPU (there is no CPU path)',
                     'x_src on the cpu': 'pygat_amd gatv2_attention: x_src must be a tensor on the GPU (there is no CPU path)',
                     'x_src float64': 'pygat_amd gatv2_attention: x_src must be float32, not torch.float64',
                     'x_src torch.bfloat16': 'pygat_amd gatv2_attention: x_src must be float32, not torch.bfloat16',
                     'x_src one more dimension': 'pygat_amd gatv2_attention: x_src (7, 2, 8, 1) does not match x_dst (5, 2, 8): the same number of '
                                                 'heads and the same width expected',
                     'x_src of 3 heads': 'pygat_amd gatv2_attention: x_src (7, 3, 8) does not match x_dst (5, 2, 8): the same number of heads and '
                                         'the same width expected',
                     'x_src of F = 4': 'pygat_amd gatv2_attention: x_src (7, 2, 4) does not match x_dst (5, 2, 8): the same number of heads and the '
                                       'same width expected',
                     'x_src one more row': 'pygat_amd gatv2_attention: x_src has 8 rows but the pattern has 7 columns',
                     'v no tensor': 'pygat_amd gatv2_attention: v must be a tensor on the GPU (there is no CPU path)',
                     'v on the cpu': 'pygat_amd gatv2_attention: v must be a tensor on the GPU (there is no CPU path)',
                     'v float64': 'pygat_amd gatv2_attention: v must be float32, not torch.float64',
                     'v torch.bfloat16': 'pygat_amd gatv2_attention: v must be float32, not torch.bfloat16',
                     'v one more dimension': 'pygat_amd gatv2_attention: v (7, 2, 8, 1) does not match x_dst (5, 2, 8): the same number of heads and '
                                             'the same width expected',
                     'v of 3 heads': 'pygat_amd gatv2_attention: v (7, 3, 8) does not match x_dst (5, 2, 8): the same number of heads and the same '
                                     'width expected',
                     'v of F = 4': 'pygat_amd gatv2_attention: v (7, 2, 4) does not match x_dst (5, 2, 8): the same number of heads and the same '
                                   'width expected',
                     'v one more row': 'pygat_amd gatv2_attention: v has 8 rows but the pattern has 7 columns',
                     'H = 65': 'pygat_amd gatv2_attention: H = 65 heads: the limits are 1 <= H <= 64',
                     'F = 12': "pygat_amd gatv2_attention: F = 12: a head's width must be a power of two in 4..256; zero-pad the columns of all four "
                               'tensors (x_dst, x_src, a and v) to the next allowed F: zero columns of a add nothing to a score, and the first F '
                               'columns of the result are unchanged',
                     'F = 2': "pygat_amd gatv2_attention: F = 2: a head's width must be a power of two in 4..256; zero-pad the columns of all four "
                              'tensors (x_dst, x_src, a and v) to the next allowed F: zero columns of a add nothing to a score, and the first F '
                              'columns of the result are unchanged',
                     'F = 512': "pygat_amd gatv2_attention: F = 512: a head's width must be a power of two in 4..256; zero-pad the columns of all "
                                'four tensors (x_dst, x_src, a and v) to the next allowed F: zero columns of a add nothing to a score, and the first '
                                'F columns of the result are unchanged',
                     'H * F = 2048': 'pygat_amd gatv2_attention: H * F = 8 * 256 = 2048 floats per row: the limit is H * F <= 1024; zero-pad the '
                                     'columns of all four tensors (x_dst, x_src, a and v) to the next allowed F: zero columns of a add nothing to a '
                                     'score, and the first F columns of the result are unchanged',
                     'negative_slope True': 'pygat_amd gatv2_attention: negative_slope = True: a finite float expected',
                     'negative_slope inf': 'pygat_amd gatv2_attention: negative_slope = inf: a finite float expected'},
 'gatv2_attention.shared': {'no pattern': 'pygat_amd gatv2_attention: an EdgePattern expected (EdgePattern.from_indices, CSRGraph.edge_pattern)',
                            'another device': 'pygat_amd gatv2_attention: x_dst lives on cpu, the pattern on cuda:1',
                            'x_dst no tensor': 'pygat_amd gatv2_attention: x_dst must be a tensor on the GPU (there is no CPU path)',
                            'x_dst on the cpu': 'pygat_amd gatv2_attention: x_dst must be a tensor on the GPU (there is no CPU path)',
                            'x_dst float64': 'pygat_amd gatv2_attention: x_dst must be float32, not torch.float64',
                            'x_dst torch.bfloat16': 'pygat_amd gatv2_attention: x_dst must be float32, not torch.bfloat16',
                            'x_dst one more dimension': 'pygat_amd gatv2_attention: x_dst [n_rows, F] or [n_rows, H, F] expected, got (5, 2, 8, 1)',
                            'x_dst of 3 heads': 'pygat_amd gatv2_attention: x_src (7, 2, 8) does not match x_dst (5, 3, 8): the same number of heads '
                                                'and the same width expected',
                            'x_dst of F = 4': 'pygat_amd gatv2_attention: x_src (7, 2, 8) does not match x_dst (5, 2, 4): the same number of heads '
                                              'and the same width expected',
                            'x_dst one more row': 'pygat_amd gatv2_attention: x_dst has 6 rows but the pattern has 5 rows',
                            'a no tensor': 'pygat_amd gatv2_attention: a must be a tensor on the GPU (there is no CPU path)',
                            'a on the cpu': 'pygat_amd gatv2_attention: a must be a tensor on the GPU (there is no CPU path)',
                            'a float64': 'pygat_amd gatv2_attention: a must be float32, not torch.float64',
                            'a torch.bfloat16': 'pygat_amd gatv2_attention: a must be float32, not torch.bfloat16',
                            'a one more dimension': 'pygat_amd gatv2_attention: a (2, 8, 1) does not match x_dst (5, 2, 8): a [F] with x_dst '
                                                    '[n_rows, F], or a [H, F] with x_dst [n_rows, H, F], expected',
                            'a of 3 heads': 'pygat_amd gatv2_attention: a (3, 8) does not match x_dst (5, 2, 8): a [F] with x_dst [n_rows, F], or a '
                                            '[H, F] with x_dst [n_rows, H, F], expected',
                            'a of F = 4': 'pygat_amd gatv2_attention: a (2, 4) does not match x_dst (5, 2, 8): a [F] with x_dst [n_rows, F], or a '
                                          '[H, F] with x_dst [n_rows, H, F], expected',
                            'x_src no tensor': 'pygat_amd gatv2_attention: x_src must be a tensor on the GPU (there is no CPU path)',
                            'x_src on the cpu': 'pygat_amd gatv2_attention: x_src must be a tensor on the GPU (there is no CPU path)',
                            'x_src float64': 'pygat_amd gatv2_attention: x_src must be float32, not torch.float64',
                            'x_src torch.bfloat16': 'pygat_amd gatv2_attention: x_src must be float32, not torch.bfloat16',
                            'x_src one more dimension': 'pygat_amd gatv2_attention: x_src (7, 2, 8, 1) does not match x_dst (5, 2, 8): the same '
                                                        'number of heads and the same width expected',
                            'x_src of 3 heads': 'pygat_amd gatv2_attention: x_src (7, 3, 8) does not match x_dst (5, 2, 8): the same number of heads '
                                                'and the same width expected',
                            'x_src of F = 4': 'pygat_amd gatv2_attention: x_src (7, 2, 4) does not match x_dst (5, 2, 8): the same number of heads '
                                              'and the same width expected',
                            'x_src one more row': 'pygat_amd gatv2_attention: x_src has 8 rows but the pattern has 7 columns',
                            'H = 65': 'pygat_amd gatv2_attention: H = 65 heads: the limits are 1 <= H <= 64',
                            'F = 12': "pygat_amd gatv2_attention: F = 12: a head's width must be a power of two in 4..256; zero-pad the columns of "
                                      'all four tensors (x_dst, x_src, a and v) to the next allowed F: zero columns of a add nothing to a score, and '
                                      'the first F columns of the result are unchanged',
                            'F = 2': "pygat_amd gatv2_attention: F = 2: a head's width must be a power of two in 4..256; zero-pad the columns of all "
                                     'four tensors (x_dst, x_src, a and v) to the next allowed F: zero columns of a add nothing to a score, and the '
                                     'first F columns of the result are unchanged',
                            'F = 512': "pygat_amd gatv2_attention: F = 512: a head's width must be a power of two in 4..256; zero-pad the columns of "
                                       'all four tensors (x_dst, x_src, a and v) to the next allowed F: zero columns of a add nothing to a score, '
                                       'and the first F columns of the result are unchanged',
                            'H * F = 2048': 'pygat_amd gatv2_attention: H * F = 8 * 256 = 2048 floats per row: the limit is H * F <= 1024; zero-pad '
                                            'the columns of all four tensors (x_dst, x_src, a and v) to the next allowed F: zero columns of a add '
                                            'nothing to a score, and the first F columns of the result are unchanged',
                            'negative_slope True': 'pygat_amd gatv2_attention: negative_slope = True: a finite float expected',
                            'negative_slope inf': 'pygat_amd gatv2_attention: negative_slope = inf: a finite float expected'},
 'gatv2_attention_dropout': {'no pattern': 'pygat_amd gatv2_attention_dropout: an EdgePattern expected (EdgePattern.from_indices, '
                                           'CSRGraph.edge_pattern)',
                             'another device': 'pygat_amd gatv2_attention_dropout: x_dst lives on cpu, the pattern on cuda:1',
                             'x_dst no tensor': 'pygat_amd gatv2_attention_dropout: x_dst must be a tensor on the GPU (there is no CPU path)',
                             'x_dst on the cpu': 'pygat_amd gatv2_attention_dropout: x_dst must be a tensor on the GPU (there is no CPU path)',
                             'x_dst float64': 'pygat_amd gatv2_attention_dropout: x_dst must be float32, not torch.float64',
                             'x_dst torch.bfloat16': 'pygat_amd gatv2_attention_dropout: x_dst, x_src, a and v must be float32: there is no training '
                                                     'path on bfloat16 tensors',
                             'x_dst one more dimension': 'pygat_amd gatv2_attention_dropout: x_dst [n_rows, F] or [n_rows, H, F] expected, got (5, '
                                                         '2, 8, 1)',
                             'x_dst of 3 heads': 'pygat_amd gatv2_attention_dropout: x_src (7, 2, 8) does not match x_dst (5, 3, 8): the same number '
                                                 'of heads and the same width expected',
                             'x_dst of F = 4': 'pygat_amd gatv2_attention_dropout: x_src (7, 2, 8) does not match x_dst (5, 2, 4): the same number '
                                               'of heads and the same width expected',
                             'x_dst one more row': 'pygat_amd gatv2_attention_dropout: x_dst has 6 rows but the pattern has 5 rows',
                             'a no tensor': 'pygat_amd gatv2_attention_dropout: a must be a tensor on the GPU (there is no CPU path)',
                             'a on the cpu': 'pygat_amd gatv2_attention_dropout: a must be a tensor on the GPU (there is no CPU path)',
                             'a float64': 'pygat_amd gatv2_attention_dropout: a must be float32, not torch.float64',
                             'a torch.bfloat16': 'pygat_amd gatv2_attention_dropout: x_dst, x_src, a and v must be float32: there is no training '
                                                 'path on bfloat16 tensors',
                             'a one more dimension': 'pygat_amd gatv2_attention_dropout: a (2, 8, 1) does not match x_dst (5, 2, 8): a [F] with '
                                                     'x_dst [n_rows, F], or a [H, F] with x_dst [n_rows, H, F], expected',
                             'a of 3 heads': 'pygat_amd gatv2_attention_dropout: a (3, 8) does not match x_dst (5, 2, 8): a [F] with x_dst [n_rows, '
                                             'F], or a [H, F] with x_dst [n_rows, H, F], expected',
                             'a of F = 4': 'pygat_amd gatv2_attention_dropout: a (2, 4) does not match x_dst (5, 2, 8): a [F] with x_dst [n_rows, '
                                           'F], or a [H, F] with x_dst [n_rows, H, F], expected',
                             'x_src no tensor': 'pygat_amd gatv2_attention_dropout: x_src must be a tensor on the GPU (there is no CPU path)',
                             'x_src on the cpu': 'pygat_amd gatv2_attention_dropout: x_src must be a tensor on the GPU (there is no CPU path)',
                             'x_src float64': 'pygat_amd gatv2_attention_dropout: x_src must be float32, not torch.float64',
                             'x_src torch.bfloat16': 'pygat_amd gatv2_attention_dropout: x_dst, x_src, a and v must be float32: there is no training '
                                                     'path on bfloat16 tensors',
                             'x_src one more dimension': 'pygat_amd gatv2_attention_dropout: x_src (7, 2, 8, 1) does not match x_dst (5, 2, 8): the '
                                                         'same number of heads and the same width expected',
                             'x_src of 3 heads': 'pygat_amd gatv2_attention_dropout: x_src (7, 3, 8) does not match x_dst (5, 2, 8): the same number '
                                                 'of heads and the same width expected',
                             'x_src of F = 4': 'pygat_amd gatv2_attention_dropout: x_src (7, 2, 4) does not match x_dst (5, 2, 8): the same number '
                                               'of heads and the same width expected',
                             'x_src one more row': 'pygat_amd gatv2_attention_dropout: x_src has 8 rows but the pattern has 7 columns',
                             'v no tensor': 'pygat_amd gatv2_attention_dropout: v must be a tensor on the GPU (there is no CPU path)',
                             'v on the cpu': 'pygat_amd gatv2_attention_dropout: v must be a tensor on the GPU (there is no CPU path)',
                             'v float64': 'pygat_amd gatv2_attention_dropout: v must be float32, not torch.float64',
                             'v torch.bfloat16': 'pygat_amd gatv2_attention_dropout: x_dst, x_src, a and v must be float32: there is no training '
                                                 'path on bfloat16 tensors',
                             'v one more dimension': 'pygat_amd gatv2_attention_dropout: v (7, 2, 8, 1) does not match x_dst (5, 2, 8): the same '
                                                     'number of heads and the same width expected',
                             'v of 3 heads': 'pygat_amd gatv2_attention_dropout: v (7, 3, 8) does not match x_dst (5, 2, 8): the same number of '
                                             'heads and the same width expected',
                             'v of F = 4': 'pygat_amd gatv2_attention_dropout: v (7, 2, 4) does not match x_dst (5, 2, 8): the same number of heads '
                                           'and the same width expected',
                             'v one more row': 'pygat_amd gatv2_attention_dropout: v has 8 rows but the pattern has 7 columns',
                             'H = 65': 'pygat_amd gatv2_attention_dropout: H = 65 heads: the limits are 1 <= H <= 64',
                             'F = 12': "pygat_amd gatv2_attention_dropout: F = 12: a head's width must be a power of two in 4..256; zero-pad the "
                                       'columns of all four tensors (x_dst, x_src, a and v) to the next allowed F: zero columns of a add nothing to '
                                       'a score, and the first F columns of the result are unchanged',
                             'F = 2': "pygat_amd gatv2_attention_dropout: F = 2: a head's width must be a power of two in 4..256; zero-pad the "
                                      'columns of all four tensors (x_dst, x_src, a and v) to the next allowed F: zero columns of a add nothing to a '
                                      'score, and the first F columns of the result are unchanged',
                             'F = 512': "pygat_amd gatv2_attention_dropout: F = 512: a head's width must be a power of two in 4..256; zero-pad the "
                                        'columns of all four tensors (x_dst, x_src, a and v) to the next allowed F: zero columns of a add nothing to '
                                        'a score, and the first F columns of the result are unchanged',
                             'H * F = 2048': 'pygat_amd gatv2_attention_dropout: H * F = 8 * 256 = 2048 floats per row: the limit is H * F <= 1024; '
                                             'zero-pad the columns of all four tensors (x_dst, x_src, a and v) to the next allowed F: zero columns '
                                             'of a add nothing to a score, and the first F columns of the result are unchanged',
                             'p -0.1': 'pygat_amd gatv2_attention_dropout: p = -0.1: a dropout probability in [0, 1] expected',
                             'p 1.5': 'pygat_amd gatv2_attention_dropout: p = 1.5: a dropout probability in [0, 1] expected',
                             'p True': 'pygat_amd gatv2_attention_dropout: p = True: a dropout probability in [0, 1] expected',
                             'p nan': 'pygat_amd gatv2_attention_dropout: p = nan: a dropout probability in [0, 1] expected',
                             'seed dtype': "pygat_amd gatv2_attention_dropout: seed must be an int64 tensor of shape [1] on the pattern's device cpu "
                                           '(the kernels read it there, so a captured graph replays with the value it finds), got torch.int32 (1,) '
                                           'on cpu',
                             'seed shape': "pygat_amd gatv2_attention_dropout: seed must be an int64 tensor of shape [1] on the pattern's device cpu "
                                           '(the kernels read it there, so a captured graph replays with the value it finds), got torch.int64 (2,) '
                                           'on cpu',
                             'seed no tensor': "pygat_amd gatv2_attention_dropout: seed must be an int64 tensor of shape [1] on the pattern's device "
                                               'cpu (the kernels read it there, so a captured graph replays with the value it finds), got int',
                             'negative_slope True': 'pygat_amd gatv2_attention_dropout: negative_slope = True: a finite float expected',
                             'negative_slope inf': 'pygat_amd gatv2_attention_dropout: negative_slope = inf: a finite float expected'},
 'gatv2_attention_edge': {'no pattern': 'pygat_amd gatv2_attention_edge: an EdgePattern expected (EdgePattern.from_indices, CSRGraph.edge_pattern)',
                          'another device': 'pygat_amd gatv2_attention_edge: e lives on cpu, the pattern on cuda:1; e [E, H, F] (or [E, F] without a '
                                            "head axis), a row per entry at the caller's entry index, expected",
                          'x_dst no tensor': 'pygat_amd gatv2_attention_edge: x_dst must be a tensor on the GPU (there is no CPU path)',
                          'x_dst on the cpu': 'pygat_amd gatv2_attention_edge: x_dst must be a tensor on the GPU (there is no CPU path)',
                          'x_dst float64': 'pygat_amd gatv2_attention_edge: x_dst must be float32, not torch.float64',
                          'x_dst torch.bfloat16': 'pygat_amd gatv2_attention_edge: x_dst, x_src, a, v and e must be float32: there are no bfloat16 '
                                                  'tables in this op',
                          'x_dst one more dimension': 'pygat_amd gatv2_attention_edge: x_dst [n_rows, F] or [n_rows, H, F] expected, got (5, 2, 8, '
                                                      '1)',
                          'x_dst of 3 heads': 'pygat_amd gatv2_attention_edge: x_src (7, 2, 8) does not match x_dst (5, 3, 8): the same number of '
                                              'heads and the same width expected',
                          'x_dst of F = 4': 'pygat_amd gatv2_attention_edge: x_src (7, 2, 8) does not match x_dst (5, 2, 4): the same number of '
                                            'heads and the same width expected',
                          'x_dst one more row': 'pygat_amd gatv2_attention_edge: x_dst has 6 rows but the pattern has 5 rows',
                          'a no tensor': 'pygat_amd gatv2_attention_edge: a must be a tensor on the GPU (there is no CPU path)',
                          'a on the cpu': 'pygat_amd gatv2_attention_edge: a must be a tensor on the GPU (there is no CPU path)',
                          'a float64': 'pygat_amd gatv2_attention_edge: a must be float32, not torch.float64',
                          'a torch.bfloat16': 'pygat_amd gatv2_attention_edge: x_dst, x_src, a, v and e must be float32: there are no bfloat16 '
                                              'tables in this op',
                          'a one more dimension': 'pygat_amd gatv2_attention_edge: a (2, 8, 1) does not match x_dst (5, 2, 8): a [F] with x_dst '
                                                  '[n_rows, F], or a [H, F] with x_dst [n_rows, H, F], expected',
                          'a of 3 heads': 'pygat_amd gatv2_attention_edge: a (3, 8) does not match x_dst (5, 2, 8): a [F] with x_dst [n_rows, F], or '
                                          'a [H, F] with x_dst [n_rows, H, F], expected',
                          'a of F = 4': 'pygat_amd gatv2_attention_edge: a (2, 4) does not match x_dst (5, 2, 8): a [F] with x_dst [n_rows, F], or a '
                                        '[H, F] with x_dst [n_rows, H, F], expected',
                          'x_src no tensor': 'pygat_amd gatv2_attention_edge: x_src must be a tensor on the GPU (there is no CPU path)',
                          'x_src on the cpu': 'pygat_amd gatv2_attention_edge: x_src must be a tensor on the GPU (there is no CPU path)',
                          'x_src float64': 'pygat_amd gatv2_attention_edge: x_src must be float32, not torch.float64',
                          'x_src torch.bfloat16': 'pygat_amd gatv2_attention_edge: x_dst, x_src, a, v and e must be float32: there are no bfloat16 '
                                                  'tables in this op',
                          'x_src one more dimension': 'pygat_amd gatv2_attention_edge: x_src (7, 2, 8, 1) does not match x_dst (5, 2, 8): the same '
                                                      'number of heads and the same width expected',
                          'x_src of 3 heads': 'pygat_amd gatv2_attention_edge: x_src (7, 3, 8) does not match x_dst (5, 2, 8): the same number of '
                                              'heads and the same width expected',
                          'x_src of F = 4': 'pygat_amd gatv2_attention_edge: x_src (7, 2, 4) does not match x_dst (5, 2, 8): the same number of '
                                            'heads and the same width expected',
                          'x_src one more row': 'pygat_amd gatv2_attention_edge: x_src has 8 rows but the pattern has 7 columns',
                          'e no tensor': 'pygat_amd gatv2_attention_edge: e must be a tensor on the GPU (there is no CPU path); e [E, H, F] (or [E, '
                                         "F] without a head axis), a row per entry at the caller's entry index, expected",
                          'e on the cpu': 'pygat_amd gatv2_attention_edge: e must be a tensor on the GPU (there is no CPU path); e [E, H, F] (or [E, '
                                          "F] without a head axis), a row per entry at the caller's entry index, expected",
                          'e float64': 'pygat_amd gatv2_attention_edge: e must be float32, not torch.float64; e [E, H, F] (or [E, F] without a head '
                                       "axis), a row per entry at the caller's entry index, expected",
                          'e torch.bfloat16': 'pygat_amd gatv2_attention_edge: x_dst, x_src, a, v and e must be float32: there are no bfloat16 '
                                              'tables in this op',
                          'e one more dimension': 'pygat_amd gatv2_attention_edge: e [11, 2, 8] expected for E = 11 entries and x_dst (5, 2, 8) -- '
                                                  '(E,) + x_dst.shape[1:], a row per entry -- got (11, 2, 8, 1)',
                          'e of 3 heads': 'pygat_amd gatv2_attention_edge: e [11, 2, 8] expected for E = 11 entries and x_dst (5, 2, 8) -- (E,) + '
                                          'x_dst.shape[1:], a row per entry -- got (11, 3, 8)',
                          'e of F = 4': 'pygat_amd gatv2_attention_edge: e [11, 2, 8] expected for E = 11 entries and x_dst (5, 2, 8) -- (E,) + '
                                        'x_dst.shape[1:], a row per entry -- got (11, 2, 4)',
                          'e one more row': 'pygat_amd gatv2_attention_edge: e [11, 2, 8] expected for E = 11 entries and x_dst (5, 2, 8) -- (E,) + '
                                            'x_dst.shape[1:], a row per entry -- got (12, 2, 8)',
                          'v no tensor': 'pygat_amd gatv2_attention_edge: v must be a tensor on the GPU (there is no CPU path)',
                          'v on the cpu': 'pygat_amd gatv2_attention_edge: v must be a tensor on the GPU (there is no CPU path)',
                          'v float64': 'pygat_amd gatv2_attention_edge: v must be float32, not torch.float64',
                          'v torch.bfloat16': 'pygat_amd gatv2_attention_edge: x_dst, x_src, a, v and e must be float32: there are no bfloat16 '
                                              'tables in this op',
                          'v one more dimension': 'pygat_amd gatv2_attention_edge: v (7, 2, 8, 1) does not match x_dst (5, 2, 8): the same number of '
                                                  'heads and the same width expected',
                          'v of 3 heads': 'pygat_amd gatv2_attention_edge: v (7, 3, 8) does not match x_dst (5, 2, 8): the same number of heads and '
                                          'the same width expected',
                          'v of F = 4': 'pygat_amd gatv2_attention_edge: v (7, 2, 4) does not match x_dst (5, 2, 8): the same number of heads and '
                                        'the same width expected',
                          'v one more row': 'pygat_amd gatv2_attention_edge: v has 8 rows but the pattern has 7 columns',
                          'H = 65': 'pygat_amd gatv2_attention_edge: H = 65 heads: the limits are 1 <= H <= 64',
                          'F = 12': "pygat_amd gatv2_attention_edge: F = 12: a head's width must be a power of two in 4..256; zero-pad the columns "
                                    'of all four tensors (x_dst, x_src, a and v) to the next allowed F: zero columns of a add nothing to a score, '
                                    'and the first F columns of the result are unchanged',
                          'F = 2': "pygat_amd gatv2_attention_edge: F = 2: a head's width must be a power of two in 4..256; zero-pad the columns of "
                                   'all four tensors (x_dst, x_src, a and v) to the next allowed F: zero columns of a add nothing to a score, and '
                                   'the first F columns of the result are unchanged',
                          'F = 512': "pygat_amd gatv2_attention_edge: F = 512: a head's width must be a power of two in 4..256; zero-pad the columns "
                                     'of all four tensors (x_dst, x_src, a and v) to the next allowed F: zero columns of a add nothing to a score, '
                                     'and the first F columns of the result are unchanged',
                          'H * F = 2048': 'pygat_amd gatv2_attention_edge: H * F = 8 * 256 = 2048 floats per row: the limit is H * F <= 1024; '
                                          'zero-pad the columns of all four tensors (x_dst, x_src, a and v) to the next allowed F: zero columns of a '
                                          'add nothing to a score, and the first F columns of the result are unchanged',
                          'negative_slope True': 'pygat_amd gatv2_attention_edge: negative_slope = True: a finite float expected',
                          'negative_slope inf': 'pygat_amd gatv2_attention_edge: negative_slope = inf: a finite float expected'},
 'gatv2_attention_bf16': {'no pattern': 'pygat_amd gatv2_attention_bf16: an EdgePattern expected (EdgePattern.from_indices, CSRGraph.edge_pattern)',
                          'another device': 'pygat_amd gatv2_attention_bf16: x_dst lives on cpu, the pattern on cuda:1',
                          'x_dst no tensor': 'pygat_amd gatv2_attention_bf16: x_dst must be a tensor on the GPU (there is no CPU path)',
                          'x_dst on the cpu': 'pygat_amd gatv2_attention_bf16: x_dst must be a tensor on the GPU (there is no CPU path)',
                          'x_dst float64': 'pygat_amd gatv2_attention_bf16: x_dst must be torch.float32, not torch.float64: it is float32 in this '
                                           'op: only the row tables of H * F values are bfloat16',
                          'x_dst torch.bfloat16': 'pygat_amd gatv2_attention_bf16: x_dst must be torch.float32, not torch.bfloat16: it is float32 in '
                                                  'this op: only the row tables of H * F values are bfloat16',
                          'x_dst one more dimension': 'pygat_amd gatv2_attention_bf16: x_dst [n_rows, F] or [n_rows, H, F] expected, got (5, 2, 8, '
                                                      '1)',
                          'x_dst of 3 heads': 'pygat_amd gatv2_attention_bf16: x_src16 (7, 2, 8) does not match x_dst (5, 3, 8): the same number of '
                                              'heads and the same width expected',
                          'x_dst of F = 4': 'pygat_amd gatv2_attention_bf16: x_src16 (7, 2, 8) does not match x_dst (5, 2, 4): the same number of '
                                            'heads and the same width expected',
                          'x_dst one more row': 'pygat_amd gatv2_attention_bf16: x_dst has 6 rows but the pattern has 5 rows',
                          'a no tensor': 'pygat_amd gatv2_attention_bf16: a must be a tensor on the GPU (there is no CPU path)',
                          'a on the cpu': 'pygat_amd gatv2_attention_bf16: a must be a tensor on the GPU (there is no CPU path)',
                          'a float64': 'pygat_amd gatv2_attention_bf16: a must be torch.float32, not torch.float64: it is float32 in this op: only '
                                       'the row tables of H * F values are bfloat16',
                          'a torch.bfloat16': 'pygat_amd gatv2_attention_bf16: a must be torch.float32, not torch.bfloat16: it is float32 in this '
                                              'op: only the row tables of H * F values are bfloat16',
                          'a one more dimension': 'pygat_amd gatv2_attention_bf16: a (2, 8, 1) does not match x_dst (5, 2, 8): a [F] with x_dst '
                                                  '[n_rows, F], or a [H, F] with x_dst [n_rows, H, F], expected',
                          'a of 3 heads': 'pygat_amd gatv2_attention_bf16: a (3, 8) does not match x_dst (5, 2, 8): a [F] with x_dst [n_rows, F], or '
                                          'a [H, F] with x_dst [n_rows, H, F], expected',
                          'a of F = 4': 'pygat_amd gatv2_attention_bf16: a (2, 4) does not match x_dst (5, 2, 8): a [F] with x_dst [n_rows, F], or a '
                                        '[H, F] with x_dst [n_rows, H, F], expected',
                          'x_src16 no tensor': 'pygat_amd gatv2_attention_bf16: x_src16 must be a tensor on the GPU (there is no CPU path)',
                          'x_src16 on the cpu': 'pygat_amd gatv2_attention_bf16: x_src16 must be a tensor on the GPU (there is no CPU path)',
                          'x_src16 float64': 'pygat_amd gatv2_attention_bf16: x_src16 must be torch.bfloat16, not torch.float64: it is a bfloat16 '
                                             'table of this op (make it once: t.bfloat16())',
                          'x_src16 torch.float32': 'pygat_amd gatv2_attention_bf16: x_src16 must be torch.bfloat16, not torch.float32: it is a '
                                                   'bfloat16 table of this op (make it once: t.bfloat16())',
                          'x_src16 one more dimension': 'pygat_amd gatv2_attention_bf16: x_src16 (7, 2, 8, 1) does not match x_dst (5, 2, 8): the '
                                                        'same number of heads and the same width expected',
                          'x_src16 of 3 heads': 'pygat_amd gatv2_attention_bf16: x_src16 (7, 3, 8) does not match x_dst (5, 2, 8): the same number '
                                                'of heads and the same width expected',
                          'x_src16 of F = 4': 'pygat_amd gatv2_attention_bf16: x_src16 (7, 2, 4) does not match x_dst (5, 2, 8): the same number of '
                                              'heads and the same width expected',
                          'x_src16 one more row': 'pygat_amd gatv2_attention_bf16: x_src16 has 8 rows but the pattern has 7 columns',
                          'v16 no tensor': 'pygat_amd gatv2_attention_bf16: v16 must be a tensor on the GPU (there is no CPU path)',
                          'v16 on the cpu': 'pygat_amd gatv2_attention_bf16: v16 must be a tensor on the GPU (there is no CPU path)',
                          'v16 float64': 'pygat_amd gatv2_attention_bf16: v16 must be torch.bfloat16, not torch.float64: it is a bfloat16 table of '
                                         'this op (make it once: t.bfloat16())',
                          'v16 torch.float32': 'pygat_amd gatv2_attention_bf16: v16 must be torch.bfloat16, not torch.float32: it is a bfloat16 '
                                               'table of this op (make it once: t.bfloat16())',
                          'v16 one more dimension': 'pygat_amd gatv2_attention_bf16: v16 (7, 2, 8, 1) does not match x_dst (5, 2, 8): the same '
                                                    'number of heads and the same width expected',
                          'v16 of 3 heads': 'pygat_amd gatv2_attention_bf16: v16 (7, 3, 8) does not match x_dst (5, 2, 8): the same number of heads '
                                            'and the same width expected',
                          'v16 of F = 4': 'pygat_amd gatv2_attention_bf16: v16 (7, 2, 4) does not match x_dst (5, 2, 8): the same number of heads '
                                          'and the same width expected',
                          'v16 one more row': 'pygat_amd gatv2_attention_bf16: v16 has 8 rows but the pattern has 7 columns',
                          'H = 65': 'pygat_amd gatv2_attention_bf16: H = 65 heads: the limits are 1 <= H <= 64',
                          'F = 12': "pygat_amd gatv2_attention_bf16: F = 12: a head's width must be a power of two in 4..256; zero-pad the columns "
                                    'of all four tensors (x_dst, x_src, a and v) to the next allowed F: zero columns of a add nothing to a score, '
                                    'and the first F columns of the result are unchanged',
                          'F = 2': "pygat_amd gatv2_attention_bf16: F = 2: a head's width must be a power of two in 4..256; zero-pad the columns of "
                                   'all four tensors (x_dst, x_src, a and v) to the next allowed F: zero columns of a add nothing to a score, and '
                                   'the first F columns of the result are unchanged',
                          'F = 512': "pygat_amd gatv2_attention_bf16: F = 512: a head's width must be a power of two in 4..256; zero-pad the columns "
                                     'of all four tensors (x_dst, x_src, a and v) to the next allowed F: zero columns of a add nothing to a score, '
                                     'and the first F columns of the result are unchanged',
                          'H * F = 2048': 'pygat_amd gatv2_attention_bf16: H * F = 8 * 256 = 2048 floats per row: the limit is H * F <= 1024; '
                                          'zero-pad the columns of all four tensors (x_dst, x_src, a and v) to the next allowed F: zero columns of a '
                                          'add nothing to a score, and the first F columns of the result are unchanged',
                          'negative_slope True': 'pygat_amd gatv2_attention_bf16: negative_slope = True: a finite float expected',
                          'negative_slope inf': 'pygat_amd gatv2_attention_bf16: negative_slope = inf: a finite float expected',
                          'x_dst requires grad': 'pygat_amd gatv2_attention_bf16: bfloat16 tables are for inference (there is no backward through '
                                                 'this op) and an argument requires grad: call it under torch.no_grad(), or use gatv2_attention on '
                                                 'float32 tables',
                          'a requires grad': 'pygat_amd gatv2_attention_bf16: bfloat16 tables are for inference (there is no backward through this '
                                             'op) and an argument requires grad: call it under torch.no_grad(), or use gatv2_attention on float32 '
                                             'tables',
                          'x_src16 requires grad': 'pygat_amd gatv2_attention_bf16: bfloat16 tables are for inference (there is no backward through '
                                                   'this op) and an argument requires grad: call it under torch.no_grad(), or use gatv2_attention on '
                                                   'float32 tables',
                          'v16 requires grad': 'pygat_amd gatv2_attention_bf16: bfloat16 tables are for inference (there is no backward through this '
                                               'op) and an argument requires grad: call it under torch.no_grad(), or use gatv2_attention on float32 '
                                               'tables'},
 'gatv2_attention_edge_bf16': {'no pattern': 'pygat_amd gatv2_attention_edge_bf16: an EdgePattern expected (EdgePattern.from_indices, '
                                             'CSRGraph.edge_pattern)',
                               'another device': 'pygat_amd gatv2_attention_edge_bf16: e16 lives on cpu, the pattern on cuda:1; e [E, H, F] (or [E, '
                                                 "F] without a head axis), a row per entry at the caller's entry index, expected",
                               'x_dst no tensor': 'pygat_amd gatv2_attention_edge_bf16: x_dst must be a tensor on the GPU (there is no CPU path)',
                               'x_dst on the cpu': 'pygat_amd gatv2_attention_edge_bf16: x_dst must be a tensor on the GPU (there is no CPU path)',
                               'x_dst float64': 'pygat_amd gatv2_attention_edge_bf16: x_dst must be torch.float32, not torch.float64: it is float32 '
                                                'in this op: only the row tables of H * F values are bfloat16',
                               'x_dst torch.bfloat16': 'pygat_amd gatv2_attention_edge_bf16: x_dst must be torch.float32, not torch.bfloat16: it is '
                                                       'float32 in this op: only the row tables of H * F values are bfloat16',
                               'x_dst one more dimension': 'pygat_amd gatv2_attention_edge_bf16: x_dst [n_rows, F] or [n_rows, H, F] expected, got '
                                                           '(5, 2, 8, 1)',
                               'x_dst of 3 heads': 'pygat_amd gatv2_attention_edge_bf16: x_src16 (7, 2, 8) does not match x_dst (5, 3, 8): the same '
                                                   'number of heads and the same width expected',
                               'x_dst of F = 4': 'pygat_amd gatv2_attention_edge_bf16: x_src16 (7, 2, 8) does not match x_dst (5, 2, 4): the same '
                                                 'number of heads and the same width expected',
                               'x_dst one more row': 'pygat_amd gatv2_attention_edge_bf16: x_dst has 6 rows but the pattern has 5 rows',
                               'a no tensor': 'pygat_amd gatv2_attention_edge_bf16: a must be a tensor on the GPU (there is no CPU path)',
                               'a on the cpu': 'pygat_amd gatv2_attention_edge_bf16: a must be a tensor on the GPU (there is no CPU path)',
                               'a float64': 'pygat_amd gatv2_attention_edge_bf16: a must be torch.float32, not torch.float64: it is float32 in this '
                                            'op: only the row tables of H * F values are bfloat16',
                               'a torch.bfloat16': 'pygat_amd gatv2_attention_edge_bf16: a must be torch.float32, not torch.bfloat16: it is float32 '
                                                   'in this op: only the row tables of H * F values are bfloat16',
                               'a one more dimension': 'pygat_amd gatv2_attention_edge_bf16: a (2, 8, 1) does not match x_dst (5, 2, 8): a [F] with '
                                                       'x_dst [n_rows, F], or a [H, F] with x_dst [n_rows, H, F], expected',
                               'a of 3 heads': 'pygat_amd gatv2_attention_edge_bf16: a (3, 8) does not match x_dst (5, 2, 8): a [F] with x_dst '
                                               '[n_rows, F], or a [H, F] with x_dst [n_rows, H, F], expected',
                               'a of F = 4': 'pygat_amd gatv2_attention_edge_bf16: a (2, 4) does not match x_dst (5, 2, 8): a [F] with x_dst '
                                             '[n_rows, F], or a [H, F] with x_dst [n_rows, H, F], expected',
                               'x_src16 no tensor': 'pygat_amd gatv2_attention_edge_bf16: x_src16 must be a tensor on the GPU (there is no CPU path)',
                               'x_src16 on the cpu': 'pygat_amd gatv2_attention_edge_bf16: x_src16 must be a tensor on the GPU (there is no CPU '
                                                     'path)',
                               'x_src16 float64': 'pygat_amd gatv2_attention_edge_bf16: x_src16 must be torch.bfloat16, not torch.float64: it is a '
                                                  'bfloat16 table of this op (make it once: t.bfloat16())',
                               'x_src16 torch.float32': 'pygat_amd gatv2_attention_edge_bf16: x_src16 must be torch.bfloat16, not torch.float32: it '
                                                        'is a bfloat16 table of this op (make it once: t.bfloat16())',
                               'x_src16 one more dimension': 'pygat_amd gatv2_attention_edge_bf16: x_src16 (7, 2, 8, 1) does not match x_dst (5, 2, '
                                                             '8): the same number of heads and the same width expected',
                               'x_src16 of 3 heads': 'pygat_amd gatv2_attention_edge_bf16: x_src16 (7, 3, 8) does not match x_dst (5, 2, 8): the '
                                                     'same number of heads and the same width expected',
                               'x_src16 of F = 4': 'pygat_amd gatv2_attention_edge_bf16: x_src16 (7, 2, 4) does not match x_dst (5, 2, 8): the same '
                                                   'number of heads and the same width expected',
                               'x_src16 one more row': 'pygat_amd gatv2_attention_edge_bf16: x_src16 has 8 rows but the pattern has 7 columns',
                               'e16 no tensor': 'pygat_amd gatv2_attention_edge_bf16: e16 must be a tensor on the GPU (there is no CPU path); e [E, '
                                                "H, F] (or [E, F] without a head axis), a row per entry at the caller's entry index, expected",
                               'e16 on the cpu': 'pygat_amd gatv2_attention_edge_bf16: e16 must be a tensor on the GPU (there is no CPU path); e [E, '
                                                 "H, F] (or [E, F] without a head axis), a row per entry at the caller's entry index, expected",
                               'e16 float64': 'pygat_amd gatv2_attention_edge_bf16: e16 must be torch.bfloat16, not torch.float64: it is a bfloat16 '
                                              'table of this op (make it once: t.bfloat16())',
                               'e16 torch.float32': 'pygat_amd gatv2_attention_edge_bf16: e16 must be torch.bfloat16, not torch.float32: it is a '
                                                    'bfloat16 table of this op (make it once: t.bfloat16())',
                               'e16 one more dimension': 'pygat_amd gatv2_attention_edge_bf16: e16 [11, 2, 8] expected for E = 11 entries and x_dst '
                                                         '(5, 2, 8) -- (E,) + x_dst.shape[1:], a row per entry -- got (11, 2, 8, 1)',
                               'e16 of 3 heads': 'pygat_amd gatv2_attention_edge_bf16: e16 [11, 2, 8] expected for E = 11 entries and x_dst (5, 2, '
                                                 '8) -- (E,) + x_dst.shape[1:], a row per entry -- got (11, 3, 8)',
                               'e16 of F = 4': 'pygat_amd gatv2_attention_edge_bf16: e16 [11, 2, 8] expected for E = 11 entries and x_dst (5, 2, 8) '
                                               '-- (E,) + x_dst.shape[1:], a row per entry -- got (11, 2, 4)',
                               'e16 one more row': 'pygat_amd gatv2_attention_edge_bf16: e16 [11, 2, 8] expected for E = 11 entries and x_dst (5, 2, '
                                                   '8) -- (E,) + x_dst.shape[1:], a row per entry -- got (12, 2, 8)',
                               'v16 no tensor': 'pygat_amd gatv2_attention_edge_bf16: v16 must be a tensor on the GPU (there is no CPU path)',
                               'v16 on the cpu': 'pygat_amd gatv2_attention_edge_bf16: v16 must be a tensor on the GPU (there is no CPU path)',
                               'v16 float64': 'pygat_amd gatv2_attention_edge_bf16: v16 must be torch.bfloat16, not torch.float64: it is a bfloat16 '
                                              'table of this op (make it once: t.bfloat16())',
                               'v16 torch.float32': 'pygat_amd gatv2_attention_edge_bf16: v16 must be torch.bfloat16, not torch.float32: it is a '
                                                    'bfloat16 table of this op (make it once: t.bfloat16())',
                               'v16 one more dimension': 'pygat_amd gatv2_attention_edge_bf16: v16 (7, 2, 8, 1) does not match x_dst (5, 2, 8): the '
                                                         'same number of heads and the same width expected',
                               'v16 of 3 heads': 'pygat_amd gatv2_attention_edge_bf16: v16 (7, 3, 8) does not match x_dst (5, 2, 8): the same number '
                                                 'of heads and the same width expected',
                               'v16 of F = 4': 'pygat_amd gatv2_attention_edge_bf16: v16 (7, 2, 4) does not match x_dst (5, 2, 8): the same number '
                                               'of heads and the same width expected',
                               'v16 one more row': 'pygat_amd gatv2_attention_edge_bf16: v16 has 8 rows but the pattern has 7 columns',
                               'H = 65': 'pygat_amd gatv2_attention_edge_bf16: H = 65 heads: the limits are 1 <= H <= 64',
                               'F = 12': "pygat_amd gatv2_attention_edge_bf16: F = 12: a head's width must be a power of two in 4..256; zero-pad the "
                                         'columns of all four tensors (x_dst, x_src, a and v) to the next allowed F: zero columns of a add nothing '
                                         'to a score, and the first F columns of the result are unchanged',
                               'F = 2': "pygat_amd gatv2_attention_edge_bf16: F = 2: a head's width must be a power of two in 4..256; zero-pad the "
                                        'columns of all four tensors (x_dst, x_src, a and v) to the next allowed F: zero columns of a add nothing to '
                                        'a score, and the first F columns of the result are unchanged',
                               'F = 512': "pygat_amd gatv2_attention_edge_bf16: F = 512: a head's width must be a power of two in 4..256; zero-pad "
                                          'the columns of all four tensors (x_dst, x_src, a and v) to the next allowed F: zero columns of a add '
                                          'nothing to a score, and the first F columns of the result are unchanged',
                               'H * F = 2048': 'pygat_amd gatv2_attention_edge_bf16: H * F = 8 * 256 = 2048 floats per row: the limit is H * F <= '
                                               '1024; zero-pad the columns of all four tensors (x_dst, x_src, a and v) to the next allowed F: zero '
                                               'columns of a add nothing to a score, and the first F columns of the result are unchanged',
                               'negative_slope True': 'pygat_amd gatv2_attention_edge_bf16: negative_slope = True: a finite float expected',
                               'negative_slope inf': 'pygat_amd gatv2_attention_edge_bf16: negative_slope = inf: a finite float expected',
                               'x_dst requires grad': 'pygat_amd gatv2_attention_edge_bf16: bfloat16 tables are for inference (there is no backward '
                                                      'through this op) and an argument requires grad: call it under torch.no_grad(), or use '
                                                      'gatv2_attention_edge on float32 tables',
                               'a requires grad': 'pygat_amd gatv2_attention_edge_bf16: bfloat16 tables are for inference (there is no backward '
                                                  'through this op) and an argument requires grad: call it under torch.no_grad(), or use '
                                                  'gatv2_attention_edge on float32 tables',
                               'x_src16 requires grad': 'pygat_amd gatv2_attention_edge_bf16: bfloat16 tables are for inference (there is no '
                                                        'backward through this op) and an argument requires grad: call it under torch.no_grad(), or '
                                                        'use gatv2_attention_edge on float32 tables',
                               'e16 requires grad': 'pygat_amd gatv2_attention_edge_bf16: bfloat16 tables are for inference (there is no backward '
                                                    'through this op) and an argument requires grad: call it under torch.no_grad(), or use '
                                                    'gatv2_attention_edge on float32 tables',
                               'v16 requires grad': 'pygat_amd gatv2_attention_edge_bf16: bfloat16 tables are for inference (there is no backward '
                                                    'through this op) and an argument requires grad: call it under torch.no_grad(), or use '
                                                    'gatv2_attention_edge on float32 tables'},
 'attention_dropout_mask': {'no pattern': 'pygat_amd attention_dropout_mask: an EdgePattern expected (EdgePattern.from_indices, '
                                          'CSRGraph.edge_pattern)',
                            'another device': "pygat_amd attention_dropout_mask: seed must be an int64 tensor of shape [1] on the pattern's device "
                                              'cuda:1 (the kernels read it there, so a captured graph replays with the value it finds), got '
                                              'torch.int64 (1,) on cpu',
                            'H = 65': 'pygat_amd attention_dropout_mask: H = 65 heads: the limits are 1 <= H <= 64',
                            'H True': 'pygat_amd attention_dropout_mask: H = True heads: the limits are 1 <= H <= 64',
                            'p -0.1': 'pygat_amd attention_dropout_mask: p = -0.1: a dropout probability in [0, 1] expected',
                            'p 1.5': 'pygat_amd attention_dropout_mask: p = 1.5: a dropout probability in [0, 1] expected',
                            'p True': 'pygat_amd attention_dropout_mask: p = True: a dropout probability in [0, 1] expected',
                            'p nan': 'pygat_amd attention_dropout_mask: p = nan: a dropout probability in [0, 1] expected',
                            'seed dtype': "pygat_amd attention_dropout_mask: seed must be an int64 tensor of shape [1] on the pattern's device cpu "
                                          '(the kernels read it there, so a captured graph replays with the value it finds), got torch.int32 (1,) on '
                                          'cpu',
                            'seed shape': "pygat_amd attention_dropout_mask: seed must be an int64 tensor of shape [1] on the pattern's device cpu "
                                          '(the kernels read it there, so a captured graph replays with the value it finds), got torch.int64 (2,) on '
                                          'cpu',
                            'seed no tensor': "pygat_amd attention_dropout_mask: seed must be an int64 tensor of shape [1] on the pattern's device "
                                              'cpu (the kernels read it there, so a captured graph replays with the value it finds), got int'},
 'order': {'dot_attention: bias before q': 'pygat_amd dot_attention: bias must be float32, not torch.float64',
           "dot_attention: q's dtype before k's shape": 'pygat_amd dot_attention: q must be float32, not torch.float64',
           "dot_attention: k's shape before q's rows": 'pygat_amd dot_attention: k (7, 3, 8) does not match q (6, 2, 8): the same number of heads '
                                                       'and the same F expected',
           "dot_attention: q's rows before the bias's shape": 'pygat_amd dot_attention: q has 6 rows but the pattern has 5 rows',
           "dot_attention: F before the bias's shape": "pygat_amd dot_attention: F = 12: a head's width must be a power of two in 4..256; "
                                                       'zero-padding the columns of q, k and v to the next allowed F leaves the first F columns of '
                                                       'the result unchanged (pass scale yourself: the default follows the padded F)',
           'dot_attention: one bf16 table before no pattern': 'pygat_amd dot_attention: k is torch.bfloat16 and v is torch.float32: the inference '
                                                              'forward takes both k and v as bfloat16 tables (k.bfloat16(), v.bfloat16()); otherwise '
                                                              'both are float32',
           'dot_attention.bf16: requires grad before no pattern': 'pygat_amd dot_attention: bfloat16 k and v are for inference (there is no backward '
                                                                  'through them): call it under torch.no_grad(), or pass float32 tables',
           'dot_attention_dropout: a bf16 v before p': 'pygat_amd dot_attention_dropout: k and v must be float32: there is no training path on '
                                                       "bfloat16 tables (they are for dot_attention's inference forward)",
           'dot_attention_dropout: p before the seed': 'pygat_amd dot_attention_dropout: p = 1.5: a dropout probability in [0, 1] expected',
           'dot_attention_dropout: the seed before q': "pygat_amd dot_attention_dropout: seed must be an int64 tensor of shape [1] on the pattern's "
                                                       'device cpu (the kernels read it there, so a captured graph replays with the value it finds), '
                                                       'got torch.int64 (2,) on cpu',
           'dot_attention_dropout: q before training=False': 'pygat_amd dot_attention_dropout: q must be a tensor on the GPU (there is no CPU path)',
           'dot_attention_edge: a bf16 e before no pattern': 'pygat_amd dot_attention_edge: k, v and e must be float32: bfloat16 tables are for '
                                                             "dot_attention's inference forward",
           "dot_attention_edge: e's dtype before the bias": 'pygat_amd dot_attention_edge: e must be float32, not torch.float64; e [E, H, F] (or [E, '
                                                            "F] without a head axis), a row per entry at the caller's entry index, expected",
           "dot_attention_edge: q before e's shape": 'pygat_amd dot_attention_edge: q has 6 rows but the pattern has 5 rows',
           "dot_attention_edge: the bias's shape before e's": 'pygat_amd dot_attention_edge: bias [E, H] = [11, 2] or [E] = [11] expected for E = 11 '
                                                              'entries and H = 2 heads, got (11, 3)',
           'additive_attention: the slope before the logit': 'pygat_amd additive_attention: negative_slope = True: a finite float expected',
           'additive_attention: the logit before s_dst': 'pygat_amd additive_attention: edge_logit must be a tensor on the GPU (there is no CPU '
                                                         'path)',
           "additive_attention: v's shape before s_dst's rows": 'pygat_amd additive_attention: v (7, 3, 8) does not match s_dst (6, 2): v [n_cols, '
                                                                'F] with s_dst [n_rows], or v [n_cols, H, F] with s_dst [n_rows, H] and the same '
                                                                'number of heads, expected',
           "additive_attention: F before the logit's shape": "pygat_amd additive_attention: F = 12: a head's width must be a power of two in 4..256; "
                                                             'zero-padding the columns of v to the next allowed F leaves the first F columns of the '
                                                             'result unchanged (no scale depends on F)',
           'additive_attention_dropout: a bf16 v before p': 'pygat_amd additive_attention_dropout: s_dst, s_src, v and edge_logit must be float32: '
                                                            'there is no training path on bfloat16 tensors',
           'additive_attention_dropout: p before the slope': 'pygat_amd additive_attention_dropout: p = 1.5: a dropout probability in [0, 1] '
                                                             'expected',
           'additive_attention_dropout: the slope before the seed': 'pygat_amd additive_attention_dropout: negative_slope = True: a finite float '
                                                                    'expected',
           'additive_attention_dropout: the seed before s_dst': 'pygat_amd additive_attention_dropout: seed must be an int64 tensor of shape [1] on '
                                                                "the pattern's device cpu (the kernels read it there, so a captured graph replays "
                                                                'with the value it finds), got torch.int64 (2,) on cpu',
           'additive_attention_bf16: the slope before requires grad': 'pygat_amd additive_attention_bf16: negative_slope = True: a finite float '
                                                                      'expected',
           'additive_attention_bf16: requires grad before a float32 v16': 'pygat_amd additive_attention_bf16: bfloat16 tables are for inference '
                                                                          '(there is no backward through this op) and an argument requires grad: '
                                                                          'call it under torch.no_grad(), or use additive_attention on float32 '
                                                                          'tables',
           'additive_attention_bf16: a float32 v16 before no pattern': 'pygat_amd additive_attention_bf16: v16 must be torch.bfloat16, not '
                                                                       'torch.float32: it is a bfloat16 table of this op (make it once: '
                                                                       't.bfloat16())',
           'gatv2_attention: the slope before x_dst': 'pygat_amd gatv2_attention: negative_slope = True: a finite float expected',
           "gatv2_attention: v's shape before a's": 'pygat_amd gatv2_attention: v (7, 3, 8) does not match x_dst (5, 2, 8): the same number of heads '
                                                    'and the same width expected',
           "gatv2_attention: a's shape before x_dst's rows": 'pygat_amd gatv2_attention: a (2, 4) does not match x_dst (6, 2, 8): a [F] with x_dst '
                                                             '[n_rows, F], or a [H, F] with x_dst [n_rows, H, F], expected',
           'gatv2_attention_dropout: a bf16 a before p': 'pygat_amd gatv2_attention_dropout: x_dst, x_src, a and v must be float32: there is no '
                                                         'training path on bfloat16 tensors',
           'gatv2_attention_dropout: p before the slope': 'pygat_amd gatv2_attention_dropout: p = 1.5: a dropout probability in [0, 1] expected',
           'gatv2_attention_dropout: the slope before the seed': 'pygat_amd gatv2_attention_dropout: negative_slope = True: a finite float expected',
           'gatv2_attention_dropout: the seed before x_dst': 'pygat_amd gatv2_attention_dropout: seed must be an int64 tensor of shape [1] on the '
                                                             "pattern's device cpu (the kernels read it there, so a captured graph replays with the "
                                                             'value it finds), got torch.int64 (2,) on cpu',
           'gatv2_attention_edge: a bf16 e before the slope': 'pygat_amd gatv2_attention_edge: x_dst, x_src, a, v and e must be float32: there are '
                                                              'no bfloat16 tables in this op',
           'gatv2_attention_edge: the slope before e': 'pygat_amd gatv2_attention_edge: negative_slope = True: a finite float expected',
           "gatv2_attention_edge: e's dtype before x_dst": 'pygat_amd gatv2_attention_edge: e must be float32, not torch.float64; e [E, H, F] (or '
                                                           "[E, F] without a head axis), a row per entry at the caller's entry index, expected",
           "gatv2_attention_edge: x_dst's rows before e's shape": 'pygat_amd gatv2_attention_edge: x_dst has 6 rows but the pattern has 5 rows',
           "gatv2_attention_edge: F before e's shape": "pygat_amd gatv2_attention_edge: F = 12: a head's width must be a power of two in 4..256; "
                                                       'zero-pad the columns of all four tensors (x_dst, x_src, a and v) to the next allowed F: zero '
                                                       'columns of a add nothing to a score, and the first F columns of the result are unchanged',
           'gatv2_attention_edge_bf16: the slope before requires grad': 'pygat_amd gatv2_attention_edge_bf16: negative_slope = True: a finite float '
                                                                        'expected',
           'gatv2_attention_edge_bf16: requires grad before a float32 e16': 'pygat_amd gatv2_attention_edge_bf16: bfloat16 tables are for inference '
                                                                            '(there is no backward through this op) and an argument requires grad: '
                                                                            'call it under torch.no_grad(), or use gatv2_attention_edge on float32 '
                                                                            'tables',
           'gatv2_attention_edge_bf16: a float32 e16 before no pattern': 'pygat_amd gatv2_attention_edge_bf16: e16 must be torch.bfloat16, not '
                                                                         'torch.float32: it is a bfloat16 table of this op (make it once: '
                                                                         't.bfloat16())',
           'gatv2_attention_edge_bf16: e16 no tensor before x_dst': 'pygat_amd gatv2_attention_edge_bf16: e16 must be a tensor on the GPU (there is '
                                                                    'no CPU path); e [E, H, F] (or [E, F] without a head axis), a row per entry at '
                                                                    "the caller's entry index, expected",
           "gatv2_attention_edge_bf16: x_dst's rows before e16's shape": 'pygat_amd gatv2_attention_edge_bf16: x_dst has 6 rows but the pattern has '
                                                                         '5 rows',
           'spmm: values before b': 'pygat_amd spmm: values must be a tensor on the GPU (there is no CPU path)',
           "spmm: b's dtype before the shapes": 'pygat_amd spmm: b must be float32, not torch.float64',
           'spmm: the shapes before the entries': 'pygat_amd spmm: values [E] with b [M, F], or values [E, H] with b [M, H, F], expected; got values '
                                                  '(12, 2) and b (7, 3, 8)',
           'edge_softmax: no pattern before by': 'pygat_amd edge_softmax: an EdgePattern expected (EdgePattern.from_indices, CSRGraph.edge_pattern)',
           'edge_softmax: by before the logits': 'pygat_amd edge_softmax: by must be "row" or "col", not \'both\'',
           'edge_dot: q before k': 'pygat_amd edge_dot: q must be a tensor on the GPU (there is no CPU path)',
           "edge_dot: k's shape before q's rows": 'pygat_amd edge_dot: k (7, 3, 8) does not match q (6, 2, 8): the same number of heads and the same '
                                                  'F expected',
           'attention_dropout_mask: p before the seed before H': 'pygat_amd attention_dropout_mask: p = 1.5: a dropout probability in [0, 1] '
                                                                 'expected',
           'attention_dropout_mask: the seed before H': 'pygat_amd attention_dropout_mask: seed must be an int64 tensor of shape [1] on the '
                                                        "pattern's device cpu (the kernels read it there, so a captured graph replays with the value "
                                                        'it finds), got torch.int64 (2,) on cpu'}}


@pytest.mark.parametrize("op", list(OPS))
def test_every_refusal_word_for_word(op):
    cases = list(_cases(op))
    assert [name for name, _ in cases] == list(EXPECTED[op]), op
    for name, args in cases:
        assert _refusal(op, args) == EXPECTED[op][name], (op, name)


@pytest.mark.parametrize("case", list(ORDER))
def test_the_order_of_two_refusals(case):
    op, args = ORDER[case]
    assert _refusal(op, args()) == EXPECTED["order"][case], case
