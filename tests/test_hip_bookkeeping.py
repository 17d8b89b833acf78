"""The adaptive bookkeeping kernels of csrc/api.hip, called directly at their own seams (256- and 1024-thread reductions,
batches of 8 pointers, grid-stride caps) -- inside the trajectories they only ever see K <= 14.  Copies and index arithmetic
are compared bit for bit; the two fp64 reductions against fp64 NumPy."""
import ctypes as C

import numpy as np
import pytest
from scipy.special import logsumexp

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from gmmvi_amd.device import get_context
    return get_context()


def ops():
    from gmmvi_amd import hip_ops
    return hip_ops


@pytest.mark.parametrize("n", [1, 255, 256, 257, 1000, 5000])
def test_normalize_logw(ctx, rng, n):
    """x - logsumexp(x), the log-sum-exp in fp64: entries down to -200 and -inf, one and several strides of the 256 threads;
    within one fp32 ulp of the fp64 result rounded to fp32."""
    x = rng.uniform(-200.0, 0.0, size=n)
    x[rng.permutation(n)[: n // 7]] = -np.inf
    x[[n // 2, (n // 2 + 1) % n]] = 0.5     # the maximum twice: no result is a tiny difference of two large numbers; n = 1: finite
    x = x.astype(np.float32)
    out, xd = ctx.empty((n,)), ctx.asarray(x)
    ctx.check(ctx.lib.gmmvi_normalize_logw(ctx.handle, xd.ptr, n, out.ptr))
    got = out.numpy()
    x64 = x.astype(np.float64)
    ref = (x64 - logsumexp(x64)).astype(np.float32)
    dead = np.isneginf(x)
    np.testing.assert_array_equal(np.isneginf(got), dead)
    assert np.all(np.abs(got[~dead].astype(np.float64) - ref[~dead]) <= np.spacing(np.abs(ref[~dead])))
    if n == 1:
        assert got[0] == 0.0


def _argmax(ctx, ld, tlp, threshold):
    best, ld_dev, tlp_dev = ctx.empty((1,), np.int32), ctx.asarray(ld), ctx.asarray(tlp)      # (held until the result is read)
    ctx.check(ctx.lib.gmmvi_add_heuristic_argmax(ctx.handle, ld_dev.ptr, tlp_dev.ptr, ld.shape[0], float(threshold), best.ptr))
    return int(best.numpy()[0])


def _argmax_ref(ld, tlp, threshold):
    """component_adaptation.py: add_at_best_location / oracle/adaptation.py:70-71 in fp64."""
    ld, tlp = ld.astype(np.float64), tlp.astype(np.float64)
    return int(np.argmax(tlp - np.maximum(ld.max() - threshold, ld)))


@pytest.mark.parametrize("n", [1, 1023, 1024, 1025, 5000])
def test_add_heuristic_argmax(ctx, rng, n):
    ld = (rng.normal(size=n) * 20 - 50).astype(np.float32)
    tlp = (rng.normal(size=n) * 20 - 60).astype(np.float32)
    for threshold in (0.0, 50.0, 1e9):                  # the floor max(ld) - threshold active for all samples, for some, for none
        active = ld.astype(np.float64).max() - threshold >= ld
        assert active.all() if threshold == 0.0 else not active.any() if threshold == 1e9 else n == 1 or 0 < active.sum() < n
        assert _argmax(ctx, ld, tlp, threshold) == _argmax_ref(ld, tlp, threshold), threshold
    # the maximum at the first and at the last index
    for at in (0, n - 1):
        t2 = tlp.copy(); t2[at] = 500.0
        assert _argmax(ctx, ld, t2, 1e9) == at == _argmax_ref(ld, t2, 1e9)
    # exact ties: the first index wins -- in different threads (i, i + 1), in the same thread (i, i + 1024), across both
    flat = np.zeros(n, np.float32)
    for pair in ((5, 6), (3, 3 + 1024), (1030, 2047), (700, 4796), (n - 2, n - 1)):
        if min(pair) < 0 or max(pair) >= n or pair[0] == pair[1]:
            continue
        t2 = np.full(n, -10.0, np.float32); t2[list(pair)] = 7.0
        assert _argmax(ctx, flat, t2, 1e9) == pair[0] == _argmax_ref(flat, t2, 1e9), pair
    assert _argmax(ctx, flat, np.full(n, 2.5, np.float32), 1e9) == 0                 # everything ties
    # tlp = -inf everywhere: every reward is -inf, argmax = 0
    assert _argmax(ctx, ld, np.full(n, -np.inf, np.float32), 50.0) == 0
    if n > 2:                                                                        # -inf everywhere but one
        t2 = np.full(n, -np.inf, np.float32); t2[n - 2] = -1e30
        assert _argmax(ctx, ld, t2, 50.0) == n - 2


@pytest.mark.parametrize("width", [1, 3, 2081])
def test_gather_rows(ctx, rng, width):
    """Repeated and descending indices; at width 2081 the 520 rows make more than 4096 x 256 words (the grid-stride loop runs a
    second time); integer payload too; no rows."""
    n_src = 300
    src = rng.normal(size=(n_src, width)).astype(np.float32) if width > 1 else rng.normal(size=n_src).astype(np.float32)
    idx = np.concatenate([np.arange(n_src - 1, -1, -1), np.full(20, 7), rng.integers(0, n_src, 200)]).astype(np.int32)
    assert idx.size * width > 4096 * 256 or width < 2081
    dsrc = ctx.asarray(src)
    np.testing.assert_array_equal(ops().gather_rows(ctx, dsrc, idx).numpy(), src[idx])
    np.testing.assert_array_equal(ops().gather_rows(ctx, dsrc, ctx.asarray(idx, np.int32)).numpy(), src[idx])
    isrc = rng.integers(-2 ** 31, 2 ** 31 - 1, size=src.shape).astype(np.int32)
    np.testing.assert_array_equal(ops().gather_rows(ctx, ctx.asarray(isrc, np.int32), idx).numpy(), isrc[idx])
    none = ops().gather_rows(ctx, dsrc, np.zeros(0, np.int32))
    assert none.shape == (0,) + src.shape[1:]
    assert ctx.lib.gmmvi_gather_rows(ctx.handle, dsrc.ptr, None, 0, width, None) == 0
    idx_dev = ctx.asarray(idx, np.int32)
    assert ctx.lib.gmmvi_gather_rows(ctx.handle, dsrc.ptr, idx_dev.ptr, -1, width, dsrc.ptr) == -2


def _copy_batch_direct(ctx, pairs):
    n = len(pairs)
    dst = (C.c_void_p * n)(*[d.ptr if d is not None else None for d, _ in pairs])
    src = (C.c_void_p * n)(*[s.ptr if s is not None else None for _, s in pairs])
    nb = (C.c_size_t * n)(*[0 if s is None else s.nbytes for _, s in pairs])
    return ctx.lib.gmmvi_copy_batch(ctx.handle, n, dst, src, nb)


@pytest.mark.parametrize("lengths", [(600001,), (1, 0, 5, 1025, 70000, 3, 256), (0, 2, 1024, 1, 99999, 7, 257, 600001)])
def test_copy_batch(ctx, rng, lengths):
    """1, 7 and 8 pairs of very different lengths in one launch (the grid is sized by the longest), empty pairs among them, and
    a length above 512 x 1024 words (the grid-stride loop); the words behind every destination stay."""
    pairs, host = [], []
    for n in lengths:
        if n == 0:
            pairs.append((None, None)); host.append(None)
            continue
        h = rng.normal(size=n).astype(np.float32)
        d = ctx.full((n + 3,), -7.0)
        pairs.append((d, ctx.asarray(h))); host.append(h)
    # (the destination is 3 words longer than the source: nbytes comes from the source)
    assert _copy_batch_direct(ctx, pairs) == 0
    for (d, _), h in zip(pairs, host):
        if h is not None:
            got = d.numpy()
            np.testing.assert_array_equal(got[:-3], h)
            np.testing.assert_array_equal(got[-3:], -7.0)


def test_copy_batch_splits_nine_pairs_and_checks_arguments(ctx, rng):
    host = [rng.normal(size=n).astype(np.float32) for n in (4, 1000, 1, 33, 2049, 17, 5, 640, 3)]
    dst = [ctx.zeros((h.size,)) for h in host]
    ops().copy_batch(ctx, [(d, ctx.asarray(h)) for d, h in zip(dst, host)] + [(ctx.empty((0,)), ctx.empty((0,)))])
    for d, h in zip(dst, host):
        np.testing.assert_array_equal(d.numpy(), h)
    with pytest.raises(ValueError):
        ops().copy_batch(ctx, [(ctx.zeros((3,)), ctx.zeros((4,)))])
    nine = [(d, ctx.asarray(h)) for d, h in zip(dst, host)]
    assert _copy_batch_direct(ctx, nine) == -2                                       # more than 8 pointers in one call
    assert ctx.lib.gmmvi_copy_batch(ctx.handle, 0, None, None, None) == 0


def test_copy_2d_sub_blocks(ctx, rng):
    """Sub-blocks with different strides on both sides, more than 256 columns (second workgroup along x); the rest stays."""
    src = rng.normal(size=(9, 700)).astype(np.float32)
    for (dr, dc, sr, sc, rows, cols) in ((2, 5, 1, 3, 6, 600), (0, 0, 0, 0, 9, 700 - 187), (10, 886, 8, 699, 1, 1), (3, 0, 0, 256, 4, 257)):
        dst = np.full((11, 887), -3.0, np.float32)
        d = ctx.asarray(dst)
        ops().copy_2d(ctx, d, dr, dc, ctx.asarray(src), sr, sc, rows, cols)
        dst[dr:dr + rows, dc:dc + cols] = src[sr:sr + rows, sc:sc + cols]
        np.testing.assert_array_equal(d.numpy(), dst)
    with pytest.raises(ValueError):
        ops().copy_2d(ctx, ctx.asarray(dst), 10, 0, ctx.asarray(src), 0, 0, 2, 5)


@pytest.mark.parametrize("rows", [1, 129, 400])
def test_remove_column(ctx, rng, rows):
    """Column idx of the first K columns of a [rows, stride] ring leaves, the later ones move left; columns from K - 1 (the stale
    last one included) and the padding up to the stride keep their contents.  129 and 400 rows: more than one workgroup."""
    k, stride = 37, 50
    a = rng.normal(size=(rows, stride)).astype(np.float32)
    for idx in (0, 17, k - 1):
        d = ctx.asarray(a)
        ctx.check(ctx.lib.gmmvi_remove_column_f32(ctx.handle, d.ptr, rows, stride, k, idx))
        ref = a.copy()
        ref[:, idx:k - 1] = a[:, idx + 1:k]
        np.testing.assert_array_equal(d.numpy(), ref)
    d = ctx.asarray(a)
    assert ctx.lib.gmmvi_remove_column_f32(ctx.handle, d.ptr, rows, stride, k, k) == -2
    assert ctx.lib.gmmvi_remove_column_f32(ctx.handle, d.ptr, rows, k - 1, k, 0) == -2
    np.testing.assert_array_equal(d.numpy(), a)


@pytest.mark.parametrize("count", [1, 1024 * 256 + 1, 2048 * 256 + 77])
def test_fill_strided_and_add_scalar(ctx, rng, count):
    """Counts above the grid caps of the two kernels (1024 and 2048 workgroups of 256): every element once, nothing else."""
    stride = 3
    buf = ctx.full((count * stride + 2,), -1.0)
    ctx.check(ctx.lib.gmmvi_fill_strided_f32(ctx.handle, buf.ptr + 4, stride, count, 2.5))      # from element 1 on
    ref = np.full(count * stride + 2, -1.0, np.float32)
    ref[1:1 + count * stride:stride] = 2.5
    np.testing.assert_array_equal(buf.numpy(), ref)
    src = rng.integers(-10 ** 9, 10 ** 9, size=count).astype(np.int32)
    dst = ctx.asarray(np.full(count + 1, 123, np.int32), np.int32)
    src_dev = ctx.asarray(src, np.int32)
    ctx.check(ctx.lib.gmmvi_add_scalar_i32(ctx.handle, dst.ptr, src_dev.ptr, -4567, count))
    got = dst.numpy()
    np.testing.assert_array_equal(got[:count], src - 4567)
    assert got[count] == 123
