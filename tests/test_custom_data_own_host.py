"""Own minibatch per sample for user-defined device targets summed over a data set, the part that needs no GPU: the per-sample
row lists of ``minibatch_stream.data_minibatch_rows_per_sample``; the keyword ``use_own_batch_per_sample`` of DeviceDataLNPDF and
DeviceDataTapeLNPDF and what reaches ``hip_ops`` with and without it; the two entries in the header and the binding; the
restatement of tests/custom_data_own_cases.py; and the planted faults, each of which moves a committed case by more than 100
times the bound of tests/test_hip_custom_data_own.py (the rule of tests/test_hip_custom_target.py, _bound)."""
import inspect
import os
import re

import numpy as np
import pytest

import custom_data_own_cases as cases
from helpers import use_host_context
from test_hip_custom_target import _bound

ALL_CASES = cases.kernel_cases()


# ---- the stream ------------------------------------------------------------------------------------------------------------
def test_row_0_is_the_shared_batch():
    from gmmvi_amd.experiments.target_distributions import minibatch_stream as ms
    for t, b in ((9, 5), (9, 9), (257, 64), (257, 257), (5, 1), (7, 2), (7, 3), (1025, 5)):
        rows = ms.data_minibatch_rows_per_sample(9, 3, 4, b, t)
        assert rows.shape == (4, b) and rows.dtype == np.int64 and rows.min() >= 0 and rows.max() < t
        np.testing.assert_array_equal(rows[0], ms.data_minibatch_rows(9, 3, b, t))
    assert ms.data_minibatch_rows_per_sample(9, 3, 0, 5, 9).shape == (0, 5)
    for bad in (0, 10):
        with pytest.raises(ValueError, match="batch_size"):
            ms.data_minibatch_rows_per_sample(9, 3, 4, bad, 9)


def test_an_epoch_is_one_permutation_cut_into_batches():
    from gmmvi_amd.experiments.target_distributions import minibatch_stream as ms
    for t, b in ((9, 5), (257, 64), (7, 2), (7, 3), (5, 1), (12, 4)):
        per_epoch = -(-t // b)                                       # ceil(T / B) batches cover an epoch
        n = 3 * per_epoch + 1
        stream = ms.data_minibatch_rows_per_sample(9, 3, n, b, t).reshape(-1)
        for e in range(3):
            epoch = stream[e * t:(e + 1) * t]
            np.testing.assert_array_equal(np.sort(epoch), np.arange(t))                  # disjoint batches that cover all rows
            np.testing.assert_array_equal(epoch, ms.permute_rows(9, 3, np.full(t, e), np.arange(t), t, stream=5))
        assert not np.array_equal(stream[:t], stream[t:2 * t])


def test_a_straddling_batch_takes_its_tail_from_the_next_epoch():
    from gmmvi_amd.experiments.target_distributions import minibatch_stream as ms
    rows = ms.data_minibatch_rows_per_sample(9, 3, 2, 5, 9)          # sample 1: positions 5 .. 9, ranks 5 .. 8 of epoch 0, rank 0 of 1
    head = ms.permute_rows(9, 3, np.zeros(4, np.int64), np.arange(5, 9), 9, stream=5)
    tail = ms.permute_rows(9, 3, np.ones(1, np.int64), np.zeros(1, np.int64), 9, stream=5)
    np.testing.assert_array_equal(rows[1], np.concatenate([head, tail]))
    assert set(rows[0]) | set(rows[1][:4]) == set(range(9))
    # such a batch may hold one row twice: over many samples it happens
    many = ms.data_minibatch_rows_per_sample(9, 3, 90, 5, 9)
    assert any(len(set(r.tolist())) < 5 for r in many)
    assert all(len(set(r.tolist())) == 5 for r in many[::9])        # a batch inside one epoch never does (9 samples = 5 epochs)


def test_full_batches_are_one_permutation_per_sample():
    from gmmvi_amd.experiments.target_distributions import minibatch_stream as ms
    for t in (9, 257):
        rows = ms.data_minibatch_rows_per_sample(9, 3, 5, t, t)
        for n in range(5):
            np.testing.assert_array_equal(np.sort(rows[n]), np.arange(t))
            np.testing.assert_array_equal(rows[n], ms.permute_rows(9, 3, np.full(t, n), np.arange(t), t, stream=5))
        assert len({tuple(r) for r in rows.tolist()}) == 5


def test_call_and_seed_change_the_lists():
    from gmmvi_amd.experiments.target_distributions import minibatch_stream as ms
    base = ms.data_minibatch_rows_per_sample(9, 3, 6, 64, 257)
    assert not np.array_equal(base, ms.data_minibatch_rows_per_sample(9, 4, 6, 64, 257))
    assert not np.array_equal(base, ms.data_minibatch_rows_per_sample(10, 3, 6, 64, 257))
    assert not np.array_equal(base, ms.minibatch_rows(9, 3, 6, 64, 257))                 # the BNN stream: another stream id
    np.testing.assert_array_equal(base, ms.data_minibatch_rows_per_sample(9, 3, 6, 64, 257))


# ---- the interface -----------------------------------------------------------------------------------------------------------
def test_symbols_and_signatures():
    from gmmvi_amd import _lib, hip_ops
    from gmmvi_amd.experiments.target_distributions.device_lnpdf import DeviceDataLNPDF, DeviceDataTapeLNPDF
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gmmvi_hip.h")).read()
    for symbol, sibling in (("gmmvi_target_custom_data_own_batches", "gmmvi_target_custom_data"),
                            ("gmmvi_target_custom_data_tape_own_batches", "gmmvi_target_custom_data_tape")):
        assert _lib.EXPORTED_SYMBOLS.count(symbol) == 1
        mine = re.search(rf"\bint {symbol}\(([^;]*)\);", header).group(1)
        theirs = re.search(rf"\bint {sibling}\(([^;]*)\);", header).group(1)
        # the sibling's argument list minus the minibatch flag
        assert re.sub(r"\s+", " ", mine) == re.sub(r"\s+", " ", theirs.replace("int minibatch, ", ""))
        assert len(_lib._PROTOS[symbol][1]) == len(_lib._PROTOS[sibling][1]) - 1
    for cls in (DeviceDataLNPDF, DeviceDataTapeLNPDF):
        names = list(inspect.signature(cls.__init__).parameters)
        assert names[names.index("seed") + 1] == "use_own_batch_per_sample"
        assert inspect.signature(cls.__init__).parameters["use_own_batch_per_sample"].default is False
    for fn in (hip_ops.target_custom_data, hip_ops.target_custom_data_tape):
        assert inspect.signature(fn).parameters["own_batches"].default is False
    assert cases.STAGED_CAP == _lib.CUSTOM_STAGED_MAX_DIM and cases.FORWARD_CAP == _lib.CUSTOM_AUTODIFF_MAX_DIM


@pytest.mark.parametrize("name", ["DeviceDataLNPDF", "DeviceDataTapeLNPDF"])
def test_class_keyword(monkeypatch, name):
    from gmmvi_amd.experiments.target_distributions import device_lnpdf
    use_host_context(monkeypatch, device_lnpdf)
    monkeypatch.setattr(device_lnpdf.hip_ops, "custom_target_compile", lambda ctx, source, **kw: object())
    monkeypatch.setattr(device_lnpdf.hip_ops, "custom_tape_length", lambda *a: 0)
    cls = getattr(device_lnpdf, name)
    op = "target_custom_data" if name == "DeviceDataLNPDF" else "target_custom_data_tape"
    seen = []

    def recording(ctx, handle, params, data, x, **kw):
        seen.append(kw)
        return np.zeros(x.shape[0], np.float32), np.zeros(x.shape, np.float32)

    monkeypatch.setattr(device_lnpdf.hip_ops, op, recording)
    data = np.zeros((9, 6), np.float32)
    with pytest.raises(ValueError, match="use_own_batch_per_sample"):
        cls(cases.SOURCES["logit"], 5, data, use_own_batch_per_sample=True)
    with pytest.raises(ValueError, match="use_own_batch_per_sample"):
        cls(cases.SOURCES["logit"], 5, data, batch_size=None, seed=3, use_own_batch_per_sample=True)
    x = np.zeros((4, 5), np.float32)
    today = {"want_grad", "batch_size", "seed", "call"} | ({"tape_capacity", "scratch_bytes"} if "tape" in op else set())
    shared = cls(cases.SOURCES["logit"], 5, data, batch_size=4, seed=3)
    assert shared.use_own_batch_per_sample is False
    shared.log_density_and_grad(x)
    shared.log_density(x)
    shared.log_density_full(x)
    assert [set(kw) for kw in seen] == [today] * 3                       # exactly today's keywords
    assert [(kw["call"], kw["batch_size"], kw["seed"]) for kw in seen] == [(0, 4, 3), (1, 4, 3), (0, None, 3)]
    del seen[:]
    own = cls(cases.SOURCES["logit"], 5, data, None, 4, 3, True)          # positionally: directly after seed
    assert own.use_own_batch_per_sample is True and own.batch_size == 4 and own.seed == 3
    own.log_density_and_grad(x)
    own.log_density(x)
    assert [set(kw) for kw in seen] == [today | {"own_batches"}] * 2     # exactly one more
    assert all(kw["own_batches"] is True for kw in seen)
    assert [(kw["call"], kw["batch_size"], kw["want_grad"]) for kw in seen] == [(0, 4, True), (1, 4, False)]
    assert own.call_count == 2
    own.log_density_full(x)                                              # all rows for every sample: the shared call
    assert set(seen[-1]) == today and seen[-1]["batch_size"] is None and own.call_count == 2


def test_operations_need_a_batch_size_for_own_batches():
    from gmmvi_amd import hip_ops
    for fn in (hip_ops.target_custom_data, hip_ops.target_custom_data_tape):
        with pytest.raises(ValueError, match="batch_size"):
            fn(None, hip_ops.CustomTarget.__new__(hip_ops.CustomTarget), None, np.zeros((9, 6), np.float32),
               np.zeros((4, 5), np.float32), own_batches=True)


# ---- the restatement -----------------------------------------------------------------------------------------------------------
def test_restatement_is_the_shared_restatement_per_sample():
    c = cases.Case("logit", 5, 7, 9, 0, 5, 3)
    tgt, x = cases.build_case(c)
    x64 = x.astype(np.float64)
    lp, g = tgt.evaluate(x64)
    lists = tgt.row_lists(7)
    for n in range(7):
        one = tgt.tgt.as_dtype(np.float64)
        one.row_list = lambda call=None, rows=lists[n]: rows
        lp_n, g_n = one.evaluate(x64[n:n + 1])
        assert lp[n] == lp_n[0] and np.array_equal(g[n], g_n[0])
    shared_lp, shared_g = tgt.tgt.evaluate(x64)                          # sample 0 sees the shared batch
    assert lp[0] == shared_lp[0] and np.array_equal(g[0], shared_g[0])
    assert np.all(lp[1:] != shared_lp[1:])
    # the counter: one step per evaluation that receives a sample
    assert tgt.call_count == 3
    tgt.log_density(x64)
    tgt.log_density_and_grad(x64)
    tgt.log_density(x64[:0])
    assert tgt.call_count == 5


@pytest.mark.parametrize("order,plan", [("waves", (1, 64)), ("waves", (3, 22)), ("tape", (1, 64)), ("tape", (3, 22))])
def test_device_orders_agree_with_the_sequence_within_the_bound(order, plan):
    c = cases.Case("logit", 17, 65, 257, 3, 64, 3)
    tgt, x, lp64, g64, lp32, g32 = cases.reference(c)
    lp, g = tgt.as_dtype(np.float32).evaluate(x, order=order, plan=plan)
    e_lp, b_lp, _ = _bound(lp, lp64, lp32)
    e_g, b_g, _ = _bound(g, g64, g32)
    assert e_lp <= b_lp and e_g <= b_g
    lp_d, g_d = tgt.evaluate(x.astype(np.float64), order=order, plan=plan)
    np.testing.assert_allclose(lp_d, lp64, rtol=1e-13)
    np.testing.assert_allclose(g_d, g64, rtol=1e-11, atol=1e-13)


def test_kernel_cases_sit_on_the_seams():
    from gmmvi_amd import _lib
    w, cap, old = _lib.CUSTOM_AUTODIFF_TANGENTS, _lib.CUSTOM_STAGED_MAX_DIM, _lib.CUSTOM_AUTODIFF_MAX_DIM
    assert {1, 63, 64, 65, 130} <= {c.n for c in ALL_CASES}
    assert {(9, 5), (9, 9), (257, 64), (257, 257), (5, 1), (7, 2), (7, 3)} <= {(c.rows, c.batch) for c in ALL_CASES}
    assert {1, w, w + 1, cap, cap + 1, old, old + 1, 1100} <= {c.d for c in ALL_CASES}
    assert {0, 1, 2, 3} <= {c.chunks for c in ALL_CASES if c.batch == 64}
    assert {"logit", "ragged"} <= {c.name for c in ALL_CASES}
    assert all(c.batch is not None for c in ALL_CASES) and len(set(ALL_CASES)) == len(ALL_CASES)
    assert cases.SLAB_CASE.n > 128 and cases.SLAB_CASE in ALL_CASES


# ---- the bound of the GPU test can see the mistakes a kernel of this kind makes ------------------------------------------------
def _applies(fault, c):
    """Whether case ``c`` can show ``fault``.  B == T: every sample's batch is all rows whatever its index or epoch, and s = 1.  A
    wrong index needs a second sample, the tile- and slab-local one a second tile (the slab here is one tile)."""
    if c.batch == c.rows:
        return False
    if fault == "scale_per_row":
        return c.batch > 1                                           # one row: s * (0 + term) is s * sum
    if fault in ("tile_local_index", "slab_local_index"):
        return c.n > 64
    return c.n > 1


@pytest.mark.parametrize("fault", cases.FAULTS)
def test_planted_fault_exceeds_a_hundred_bounds(fault):
    shown = []
    for c in ALL_CASES:
        if not _applies(fault, c):
            continue
        tgt, x, lp64, g64, lp32, g32 = cases.reference(c)
        b_lp, b_g = _bound(lp32, lp64, lp32)[1], _bound(g32, g64, g32)[1]
        lp, g = tgt.evaluate(x.astype(np.float64), fault=fault, slab=64)
        r_lp, r_g = float(np.abs(lp - lp64).max() / b_lp), float(np.abs(g - g64).max() / b_g)
        print(f"[custom_data_own] {cases.case_id(c)}: {fault} moves lp by {r_lp:.3g} and the gradient by {r_g:.3g} times the bound")
        assert max(r_lp, r_g) >= 100.0, f"{cases.case_id(c)}: {fault} moves lp by {r_lp:.3g}, the gradient by {r_g:.3g} bounds"
        shown.append(c)
    assert len(shown) >= 6, (fault, len(shown))
