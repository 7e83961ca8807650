"""Plain NumPy restatement of the seeded dropout masks (pygat_amd/csrc/rng.h, k7_dropout.hip, k9_sparse.hip): no torch,
no GPU.

Philox-4x32-10 keyed by (seed & 0xFFFFFFFF, seed >> 32), the keep rule of `make_rng`, and the three counter layouts
the kernels form:

    flat   (pygat_dropout_mask / pygat_dropout_mask2: the Wh mask and the attention mask of a level)
           element e = word (e & 3) of counter (q & 0xFFFFFFFF, q >> 32, stream, 0xFFFFFFFF), q = e >> 2
    heads  (pygat_dropout_bits, the seeded pygat_project_sparse / pygat_wgrad_sparse: rng.h draw_heads4)
           head h of x[i, k] = word (h & 3) of counter (k, i, stream, h >> 2)
    wide   (pygat_dropout_expand / pygat_dropout_head_sum with mask = NULL: rng.h draw4 over the [n, H*Fin] operand)
           column c = h*Fin + k of row i = word (c & 3) of counter (c >> 2, i, stream, 0)

rng.h says the flat and wide layouts are not part of the C ABI.  The tests pin them all the same, as a DESCRIPTION OF
THIS BUILD: everything is deterministic given the seed, so the kernels can be compared bit for bit
(tests/test_gpu_dropout_seeded.py), and the oracle run under these masks is the fp64 answer for the seeded level.  A
later change of a layout updates this file in the same commit.
"""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57          # round multipliers
K0, K1 = 0x9E3779B9, 0xBB67AE85          # key bumps
ROUNDS = 10
_LO = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def philox4x32_10(counter, key):
    """counter [..., 4], key [2] (anything that converts to unsigned 32-bit values) -> uint32 [..., 4]."""
    c = np.asarray(counter, dtype=np.uint64) & _LO
    if c.shape[-1] != 4:
        raise ValueError("philox4x32_10: the last axis of `counter` holds the four counter words")
    c0, c1, c2, c3 = (c[..., q].copy() for q in range(4))
    k0, k1 = (int(v) & 0xFFFFFFFF for v in key)
    m0, m1 = np.uint64(M0), np.uint64(M1)
    for _ in range(ROUNDS):
        p0, p1 = m0 * c0, m1 * c2             # 32 x 32 -> 64 bits: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> _S32) ^ c1 ^ np.uint64(k0), p1 & _LO, (p0 >> _S32) ^ c3 ^ np.uint64(k1), p0 & _LO
        k0, k1 = (k0 + K0) & 0xFFFFFFFF, (k1 + K1) & 0xFFFFFFFF
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def threshold(p):
    """The keep rule of rng.h make_rng -> (thresh, scale): keep iff word < thresh, kept values are scaled by `scale`.
    The C ABI takes `float p`, so keep = 1 - float32(p) in double (p = 0.6: not 0.4 * 2^32).  The clamp to 0xFFFFFFFF
    means that p = 0 drops a word equal to 0xFFFFFFFF (a 2^-32 event): mirrored here as the kernels have it."""
    p32 = float(np.float32(p))
    if not 0.0 <= p32 <= 1.0:
        raise ValueError(f"threshold: p={p} outside [0,1]")
    keep = 1.0 - p32
    thresh = min(int(keep * 4294967296.0), 0xFFFFFFFF)
    scale = np.float32(1.0 / keep) if keep > 0.0 else np.float32(0.0)
    return thresh, scale


def _key(seed):
    s = int(seed) & 0xFFFFFFFFFFFFFFFF
    return s & 0xFFFFFFFF, s >> 32


def _scaled(keep, p):
    return np.where(keep, threshold(p)[1], np.float32(0.0)).astype(np.float32)


def _flat_keep(seed, stream, count, p):
    q = np.arange((count + 3) // 4, dtype=np.uint64)
    ctr = np.stack([q & _LO, q >> _S32, np.full_like(q, int(stream) & 0xFFFFFFFF), np.full_like(q, 0xFFFFFFFF)], axis=-1)
    return philox4x32_10(ctr, _key(seed)).reshape(-1)[:count] < np.uint32(threshold(p)[0])


def flat_mask(seed, stream, count, p):
    """float32 [count], pre-scaled: the mask pygat_dropout_mask writes."""
    return _scaled(_flat_keep(seed, stream, count, p), p)


def head_keep(seed, stream, n, Fin, H, p):
    """bool [H, n, Fin]: head h keeps x[i, k]."""
    i, k = np.meshgrid(np.arange(n, dtype=np.uint64), np.arange(Fin, dtype=np.uint64), indexing="ij")
    thresh = np.uint32(threshold(p)[0])
    out = np.empty((H, n, Fin), dtype=bool)
    for hq in range((H + 3) // 4):
        ctr = np.stack([k, i, np.full_like(k, int(stream) & 0xFFFFFFFF), np.full_like(k, hq)], axis=-1)
        w = philox4x32_10(ctr, _key(seed))
        for h in range(4 * hq, min(H, 4 * hq + 4)):
            out[h] = w[..., h & 3] < thresh
    return out


def head_bits(seed, stream, n, Fin, H, p):
    """uint8 [n, Fin], bit h = head h keeps x[i, k] (H <= 8): the bytes pygat_dropout_bits writes."""
    if not 1 <= H <= 8:
        raise ValueError("head_bits: a byte holds 8 heads")
    keep = head_keep(seed, stream, n, Fin, H, p)
    bits = np.zeros((n, Fin), dtype=np.uint8)
    for h in range(H):
        bits |= keep[h].astype(np.uint8) << np.uint8(h)
    return bits


def wide_mask(seed, stream, n, Fin, H, p):
    """float32 [H, n, Fin], pre-scaled: the masks pygat_dropout_expand / pygat_dropout_head_sum draw (mask = NULL)."""
    HF = H * Fin
    i, c4 = np.meshgrid(np.arange(n, dtype=np.uint64), np.arange((HF + 3) // 4, dtype=np.uint64), indexing="ij")
    ctr = np.stack([c4, i, np.full_like(i, int(stream) & 0xFFFFFFFF), np.zeros_like(i)], axis=-1)
    keep = philox4x32_10(ctr, _key(seed)).reshape(n, -1)[:, :HF] < np.uint32(threshold(p)[0])
    return _scaled(keep.reshape(n, H, Fin).transpose(1, 0, 2), p)


def level_masks(seed, p, H, N, Fin, Fo, Fp, E, layout):
    """The three masks GATLevelDropoutFn draws from `seed`, in the oracle's shapes (pygat_amd.dropout.draw_masks):
    {"x": [H, N, Fin], "wh": [H, N, Fo], "att": [E, H]}, float32, pre-scaled.  layout = "bits" (the mask-byte and the
    sparse-feature projections) or "wide" (the wide-operand projection) decides the x masks; the Wh mask is drawn over the
    PADDED head-interleaved table [N, H*Fp], the attention mask over [E, H] in the graph's forward CSR edge order."""
    from pygat_amd.dropout import STREAM_X, STREAM_WH, STREAM_ATT
    if layout == "bits":
        x = _scaled(head_keep(seed, STREAM_X, N, Fin, H, p), p)
    elif layout == "wide":
        x = wide_mask(seed, STREAM_X, N, Fin, H, p)
    else:
        raise ValueError(f"level_masks: layout {layout!r}: expected 'bits' or 'wide'")
    wh = flat_mask(seed, STREAM_WH, N * H * Fp, p).reshape(N, H, Fp)[:, :, :Fo].transpose(1, 0, 2)
    att = flat_mask(seed, STREAM_ATT, E * H, p).reshape(E, H)
    return {"x": x, "wh": np.ascontiguousarray(wh), "att": att}
