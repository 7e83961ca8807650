"""tests/philox_ref.py on the CPU: known answers of Philox-4x32-10, the keep rule of rng.h make_rng, and the shapes and
values of the masks the reference generator builds for a level.  The GPU kernels are compared with it bit for bit in
tests/test_gpu_dropout_seeded.py."""
import numpy as np
import pytest

import philox_ref as R


@pytest.mark.parametrize("counter,key,out", [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
])
def test_known_answers(counter, key, out):
    got = R.philox4x32_10(np.array(counter, dtype=np.uint64), key)
    assert got.dtype == np.uint32 and got.shape == (4,)
    assert [int(v) for v in got] == list(out)


def test_vectorised_call_equals_single_calls():
    rng = np.random.default_rng(0)
    ctr = rng.integers(0, 1 << 32, (5, 3, 4), dtype=np.uint64)
    key = (0x12345678, 0x9abcdef0)
    got = R.philox4x32_10(ctr, key)
    assert got.shape == (5, 3, 4)
    for i in range(5):
        for j in range(3):
            assert np.array_equal(got[i, j], R.philox4x32_10(ctr[i, j], key))
    assert np.array_equal(ctr, np.asarray(ctr))                    # the caller's counters are left alone
    assert not np.array_equal(got, R.philox4x32_10(ctr, (key[0], key[1] ^ 1)))     # the high key word takes part


def test_threshold():
    assert R.threshold(1.0) == (0, np.float32(0.0))
    assert R.threshold(0.0) == (0xFFFFFFFF, np.float32(1.0))       # the clamp: a word 0xFFFFFFFF is dropped at p = 0
    assert R.threshold(0.5) == (1 << 31, np.float32(2.0))
    t01, s01 = R.threshold(0.1)
    assert t01 == int((1.0 - float(np.float32(0.1))) * 2 ** 32) and s01 == np.float32(1.0 / (1.0 - float(np.float32(0.1))))
    t06, s06 = R.threshold(0.6)
    assert t06 == int((1.0 - float(np.float32(0.6))) * 2 ** 32)
    assert t06 != int(0.4 * 2 ** 32)                                # `float p` in the C ABI: 0.6f is not 0.6
    assert s06 == np.float32(1.0 / (1.0 - float(np.float32(0.6)))) and s06.dtype == np.float32
    for p in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError):
            R.threshold(p)


def test_layouts_index_the_words_they_say():
    """Single elements of the three layouts, counters written out by hand."""
    seed, p = 0x2F00_0000_0000_0000 + 12345, 0.6
    key = (seed & 0xFFFFFFFF, seed >> 32)
    thresh, scale = R.threshold(p)
    val = lambda ctr, w: scale if int(R.philox4x32_10(np.array(ctr, dtype=np.uint64), key)[w]) < thresh else np.float32(0)  # noqa: E731
    flat = R.flat_mask(seed, 2, 23, p)
    assert flat.shape == (23,) and flat.dtype == np.float32
    for e in (0, 3, 4, 22):
        assert flat[e] == val((e >> 2, 0, 2, 0xFFFFFFFF), e & 3)
    n, Fin, H = 3, 5, 7
    bits = R.head_bits(seed, 1, n, Fin, H, p)
    assert bits.shape == (n, Fin) and bits.dtype == np.uint8 and int(bits.max()) < (1 << H)
    wide = R.wide_mask(seed, 1, n, Fin, H, p)
    assert wide.shape == (H, n, Fin) and wide.dtype == np.float32
    for i, k, h in ((0, 0, 0), (2, 4, 6), (1, 3, 4), (2, 0, 3)):
        assert ((int(bits[i, k]) >> h) & 1) == int(val((k, i, 1, h >> 2), h & 3) != 0)
        c = h * Fin + k
        assert wide[h, i, k] == val((c >> 2, i, 1, 0), c & 3)
    # both halves of the seed and the stream id take part
    assert not np.array_equal(R.flat_mask(seed, 2, 4099, p), R.flat_mask(12345, 2, 4099, p))
    assert not np.array_equal(R.flat_mask(seed, 2, 4099, p), R.flat_mask(seed, 3, 4099, p))
    assert np.array_equal(R.flat_mask(seed, 2, 4099, p)[:1023], R.flat_mask(seed, 2, 1023, p))


def test_keep_rate():
    n = 1 << 18
    for p in (0.1, 0.6):
        keep = 1.0 - p
        m = R.flat_mask(987654321, 2, n, p)
        assert abs(float((m > 0).mean()) - keep) < 5 * (keep * (1 - keep) / n) ** 0.5
    assert not R.flat_mask(1, 2, 1000, 1.0).any()
    assert (R.flat_mask(1, 2, 1000, 0.0) == 1.0).all()


@pytest.mark.parametrize("H,N,Fin,Fo,Fp", [(3, 9, 5, 5, 8), (8, 4, 7, 8, 8), (9, 5, 3, 2, 2)])
def test_level_masks(H, N, Fin, Fo, Fp):
    E, p, seed = 31, 0.6, 0x2F00_0000_0000_0000 + 12345
    scale = R.threshold(p)[1]
    both = {layout: R.level_masks(seed, p, H, N, Fin, Fo, Fp, E, layout) for layout in ("bits", "wide")}
    for m in both.values():
        assert m["x"].shape == (H, N, Fin) and m["wh"].shape == (H, N, Fo) and m["att"].shape == (E, H)   # draw_masks' shapes
        for v in m.values():
            assert v.dtype == np.float32 and np.isin(v, (np.float32(0), scale)).all() and (v == scale).any() and (v == 0).any()
    assert not np.array_equal(both["bits"]["x"], both["wide"]["x"])
    assert np.array_equal(both["bits"]["wh"], both["wide"]["wh"]) and np.array_equal(both["bits"]["att"], both["wide"]["att"])
    # the Wh mask lives on the padded head-interleaved table
    from pygat_amd.dropout import STREAM_WH, STREAM_X
    flat = R.flat_mask(seed, STREAM_WH, N * H * Fp, p)
    assert both["bits"]["wh"][H - 1, N - 1, Fo - 1] == flat[(N - 1) * H * Fp + (H - 1) * Fp + Fo - 1]
    if H <= 8:
        bits = R.head_bits(seed, STREAM_X, N, Fin, H, p)
        for h in range(H):
            assert np.array_equal(both["bits"]["x"][h] != 0, ((bits >> h) & 1).astype(bool))
    with pytest.raises(ValueError):
        R.level_masks(seed, p, H, N, Fin, Fo, Fp, E, "compact")
