"""What the CPU-only *_abi.py tests share: the library fixture, the last error message, the stand-in address, and the call of an entry
point on stand-in arguments.  What a test pins -- argtypes, the tables and scalars a launcher names, workspace formulas, the lists of
refusals -- stays in its file, and so do the stand-in arguments of a launcher that only one file calls."""
import pytest

P = 4096          # a 16-byte aligned stand-in address (never dereferenced: every call that is given it fails its checks first)


@pytest.fixture(scope="module")
def lib():
    from pygat_amd import _lib
    return _lib


def msg(L):
    return L.lib.pygat_last_error().decode()


def call(L, symbol, defaults, **kw):
    """The entry point `symbol` on its stand-in arguments `defaults`, those named in kw replaced, and a null stream."""
    assert set(kw) <= set(defaults), kw
    return getattr(L.lib, symbol)(*{**defaults, **kw}.values(), None)


# The stand-in arguments of the launchers that more than one file calls: the test of an op built on another compares its refusals
# with the wording of that op's launchers.
STAND_INS = {
    "pygat_dot_attn_forward": dict(n_rows=8, nnz=20, rowptr=P, col=P, H=2, F=8, scale=0.5, q=P, ldq=16, k=P, ldk=16, v=P, ldv=16, out=P, ldo=16,
        m=P, Z=P, ws=P),
    "pygat_dot_attn_backward_rows": dict(n_rows=8, nnz=20, rowptr=P, col=P, perm=None, H=2, F=8, scale=0.5, q=P, ldq=16, k=P, ldk=16, v=P, ldv=16,
        out=P, ldo=16, m=P, Z=P, G=P, ldg=16, dq=P, lddq=16, P=P, S=P, ws=P),
    "pygat_dot_attn_bias_forward": dict(n_rows=8, nnz=20, rowptr=P, col=P, perm=None, H=2, F=8, scale=0.5, q=P, ldq=16, k=P, ldk=16, v=P, ldv=16,
        bias=P + 4, bias_head_stride=1, out=P, ldo=16, m=P, Z=P, ws=P),
    "pygat_dot_attn_bias_backward_rows": dict(n_rows=8, nnz=20, rowptr=P, col=P, perm=None, H=2, F=8, scale=0.5, q=P, ldq=16, k=P, ldk=16, v=P,
        ldv=16, bias=P + 4, bias_head_stride=1, out=P, ldo=16, m=P, Z=P, G=P, ldg=16, dq=P, lddq=16, P=P, S=P, dbias=None, ws=P),
    "pygat_dot_attn_edge_forward": dict(n_rows=8, nnz=20, rowptr=P, col=P, perm=None, H=2, F=8, scale=0.5, q=P, ldq=16, k=P, ldk=16, v=P, ldv=16,
        e=P, lde=16, bias=P + 4, bias_head_stride=1, out=P, ldo=16, m=P, Z=P, ws=P),
    "pygat_dot_attn_edge_backward_rows": dict(n_rows=8, nnz=20, rowptr=P, col=P, perm=None, H=2, F=8, scale=0.5, q=P, ldq=16, k=P, ldk=16, v=P,
        ldv=16, e=P, lde=16, bias=P + 4, bias_head_stride=1, out=P, ldo=16, m=P, Z=P, G=P, ldg=16, dq=P, lddq=16, P=P, S=P, de=P, ldde=16,
        dbias=None, ws=P),
    "pygat_add_attn_forward": dict(n_rows=8, nnz=20, rowptr=P, col=P, perm=None, H=2, F=8, negative_slope=0.2, s_dst=P + 4, s_src=P + 4, v=P,
        ldv=16, edge_logit=P + 4, logit_head_stride=1, out=P, ldo=16, m=P, Z=P, ws=P),
    "pygat_add_attn_backward_rows": dict(n_rows=8, nnz=20, rowptr=P, col=P, perm=None, H=2, F=8, negative_slope=0.2, s_dst=P + 4, s_src=P + 4, v=P,
        ldv=16, edge_logit=P + 4, logit_head_stride=1, out=P, ldo=16, m=P, Z=P, G=P, ldg=16, ds_dst=P + 4, P=P, S=P, ws=P),
    "pygat_v2_attn_forward": dict(n_rows=8, nnz=20, rowptr=P, col=P, H=2, F=8, negative_slope=0.2, x_dst=P, ldd=16, x_src=P, lds=16, a=P, v=P,
        ldv=16, out=P, ldo=16, m=P, Z=P, ws=P),
    "pygat_v2_attn_backward_rows": dict(n_rows=8, nnz=20, rowptr=P, col=P, perm=None, H=2, F=8, negative_slope=0.2, x_dst=P, ldd=16, x_src=P,
        lds=16, a=P, v=P, ldv=16, out=P, ldo=16, m=P, Z=P, G=P, ldg=16, dx_dst=P, lddx=16, P=P, S=P, ws=P),
    "pygat_v2_attn_backward_cols": dict(n_cols=8, nnz=20, rowptr_t=P, row_t=P, perm_t=None, H=2, F=8, negative_slope=0.2, x_dst=P, ldd=16, x_src=P,
        lds=16, a=P, S=P, dx_src=P, lddx=16, da=P, ws=P),
    "pygat_v2_attn_edge_forward": dict(n_rows=8, nnz=20, rowptr=P, col=P, perm=None, H=2, F=8, negative_slope=0.2, x_dst=P, ldd=16, x_src=P, lds=16,
        a=P, v=P, ldv=16, e=P, lde=16, out=P, ldo=16, m=P, Z=P, ws=P),
    "pygat_v2_attn_edge_backward_rows": dict(n_rows=8, nnz=20, rowptr=P, col=P, perm=None, H=2, F=8, negative_slope=0.2, x_dst=P, ldd=16, x_src=P,
        lds=16, a=P, v=P, ldv=16, e=P, lde=16, out=P, ldo=16, m=P, Z=P, G=P, ldg=16, dx_dst=P, lddx=16, P=P, S=P, de=P, ldde=16, ws=P),
    "pygat_v2_attn_edge_backward_cols": dict(n_cols=8, nnz=20, rowptr_t=P, row_t=P, perm_t=None, H=2, F=8, negative_slope=0.2, x_dst=P, ldd=16,
        x_src=P, lds=16, a=P, e=P, lde=16, S=P, dx_src=P, lddx=16, da=P, ws=P),
}


def launchers(*names):
    """-> ((fn(L, **kw), name), ...): the call of pygat_<name> on its stand-in arguments, and the name its messages start with."""
    def launcher(symbol):
        def fn(L, **kw):
            return call(L, symbol, STAND_INS[symbol], **kw)
        return fn
    return tuple((launcher("pygat_" + n), n) for n in names)


DOT = launchers("dot_attn_forward", "dot_attn_backward_rows")
DOT_BIAS = launchers("dot_attn_bias_forward", "dot_attn_bias_backward_rows")
DOT_EDGE = launchers("dot_attn_edge_forward", "dot_attn_edge_backward_rows")
ADDITIVE = launchers("add_attn_forward", "add_attn_backward_rows")
GATV2 = launchers("v2_attn_forward", "v2_attn_backward_rows", "v2_attn_backward_cols")
GATV2_EDGE = launchers("v2_attn_edge_forward", "v2_attn_edge_backward_rows", "v2_attn_edge_backward_cols")
