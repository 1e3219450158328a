"""The scenarios of tests/image_script.py on the device: the same generator and the
same expectations test_image_cpu.py runs over the CPU device fake, through the
real library with copies 1 and 2 (with 2: commits and plain applies alternate).

At every check step each of these is compared exactly with the oracle's answer
the step carries, no topic left out: the host CSR on the two-phase path
(TM_DEBUG_PHASES 1), the host CSR on the one-launch kernel with 16 and with 8
lanes per topic (TM_DEBUG_SMALL_KERNEL 1 / 3; TM_DEBUG_PATH_PHASES /
TM_DEBUG_PATH_SMALL must show that each batch took the path meant), the device
pairs (tm_match_batch_dev_pairs) and tm_first_batch.  TM_DEBUG_HINT_AUDIT must
be 0.  mfcheck steps compare tm_matches_filter with Oracle.matches_filter.
"""
import numpy as np
import pytest

import image_script
from emqx_amd import _native

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return torch


def _same_csr(step, hit, vals, err, what):
    want_err = np.where(step.cnt < 0, -step.cnt, 0)
    bad = np.nonzero(err.astype(np.int64) != want_err)[0]
    assert len(bad) == 0, f"{what}: err flag of {step.topics[int(bad[0])][:80]!r}: {int(err[bad[0]])}, oracle {int(want_err[bad[0]])}"
    bad = np.nonzero(hit.astype(np.uint64) != step.hit)[0]
    assert len(bad) == 0, f"{what}: hit offsets differ from topic {step.topics[max(int(bad[0]) - 1, 0)][:80]!r}: " \
                          f"gpu {int(hit[bad[0]])} oracle {int(step.hit[bad[0]])}"
    bad = np.nonzero(vals[:len(step.vals)] != step.vals)[0]
    assert len(bad) == 0, f"{what}: {len(bad)} of {len(step.vals)} values differ, first at {int(bad[0])}"


def _check(torch, ix, step, what):
    assert ix.debug_get(_native.TM_DEBUG_HINT_AUDIT) == 0, f"{what}: hints and child slots disagree in the host image"
    n, total = len(step.topics), len(step.vals)
    for phases, kind, name in ((1, _native.SMALL_AUTO, "two phases"), (0, _native.SMALL_WAVE, "one launch, 16 lanes"),
                               (0, _native.SMALL_WAVE8, "one launch, 8 lanes")):
        ix.debug_set(_native.TM_DEBUG_PHASES, phases)
        ix.debug_set(_native.TM_DEBUG_SMALL_KERNEL, kind)
        out = (np.zeros(n + 1, np.uint64), np.zeros(total + 1024, np.uint32), np.zeros(max(n, 1), np.uint8))
        keys = (_native.TM_DEBUG_PATH_PHASES, _native.TM_DEBUG_PATH_SMALL)
        before = [ix.debug_get(k) for k in keys]
        hit, vals, err = ix.match_batch(step.blob, step.offs, out=out)
        took = [ix.debug_get(k) - b for k, b in zip(keys, before)]
        # (2 of the meant kind: the batch ran again after its staging buffer grew)
        assert took in (([1, 0], [2, 0]) if phases else ([0, 1], [0, 2])), \
            f"{what}: {name}: launches per path (phases, one launch) {took}"
        _same_csr(step, hit, vals, err, f"{what}: host CSR, {name}")
    ix.debug_set(_native.TM_DEBUG_SMALL_KERNEL, _native.SMALL_AUTO)
    # match/2
    fv, ff = ix.first_batch(step.blob, step.offs)
    bad = np.nonzero(ff != step.found)[0]
    assert len(bad) == 0, f"{what}: first_batch found code of {step.topics[int(bad[0])][:80]!r}: {int(ff[bad[0]])}, oracle {int(step.found[bad[0]])}"
    has = step.found == 1
    bad = np.nonzero(fv[has] != step.first[has])[0]
    assert len(bad) == 0, f"{what}: first_batch: {len(bad)} first values differ"
    # the device pairs
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    d_blob = torch.from_numpy(step.blob.copy()).to(dev)
    d_offs = torch.from_numpy(step.offs.view(np.int64).copy()).to(dev)
    cap = 2 * total + 4096
    d_vals = torch.zeros(cap, dtype=torch.int32, device=dev)
    d_err = torch.zeros(max(n, 1), dtype=torch.uint8, device=dev)
    d_pairs = torch.zeros(2 * n + 2, dtype=torch.int32, device=dev)
    ix.match_batch_dev_pairs(n, d_blob.data_ptr(), d_offs.data_ptr(), d_pairs.data_ptr(), d_vals.data_ptr(), cap, d_err.data_ptr(),
                             stream)
    torch.cuda.synchronize()
    pr = d_pairs.cpu().numpy().view(np.uint32).astype(np.int64)
    pv = d_vals.cpu().numpy().view(np.uint32)
    want_err = np.where(step.cnt < 0, -step.cnt, 0)
    assert np.array_equal(d_err.cpu().numpy()[:n].astype(np.int64), want_err), f"{what}: pairs err flags"
    assert int(pr[2 * n]) == total, f"{what}: pairs total {int(pr[2 * n])}, oracle {total}"
    want_cnt = np.diff(step.hit.astype(np.int64))
    bad = np.nonzero(pr[1:2 * n:2] != want_cnt)[0]
    assert len(bad) == 0, f"{what}: pairs: count of {step.topics[int(bad[0])][:80]!r}: {int(pr[2 * bad[0] + 1])}, oracle {int(want_cnt[bad[0]])}"
    pos = np.repeat(pr[0:2 * n:2] - step.hit[:-1].astype(np.int64), want_cnt) + np.arange(total)
    assert total == 0 or (pos.min() >= 0 and pos.max() < cap), f"{what}: pairs: a span leaves the values"
    bad = np.nonzero(pv[pos] != step.vals)[0]
    assert len(bad) == 0, f"{what}: pairs: {len(bad)} of {total} values differ"


def _mfcheck(ix, step, what):
    hit, vals, err = ix.matches_filter_batch(step.blob, step.offs)
    assert not err.any(), f"{what}: err flags"
    bad = np.nonzero(hit != step.hit)[0]
    assert len(bad) == 0, f"{what}: offsets differ from filter {step.topics[max(int(bad[0]) - 1, 0)]!r}"
    assert np.array_equal(vals, step.vals), f"{what}: values differ"


@pytest.mark.parametrize("copies", [1, 2])
@pytest.mark.parametrize("name", list(image_script.SCENARIOS))
def test_scenario_on_the_device(torch_dev, name, copies):
    scn = image_script.SCENARIOS[name]()
    ix = _native.Index(copies=copies)
    deltas = checks = 0
    try:
        for k, s in enumerate(scn.steps):
            what = f"{name} step {k + 1} (copies {copies})"
            if s.kind in ("apply", "commit"):
                commit = deltas % 2 == 0 if copies > 1 else s.kind == "commit"
                ix.apply(s.ops, s.blob, s.offs, s.vals, s.flags, commit=commit)
                deltas += 1
            elif s.kind == "check":
                _check(torch_dev, ix, s, f"{what}: {s.label}")
                checks += 1
            else:
                _mfcheck(ix, s, f"{what}: {s.label}")
        assert checks == sum(s.kind == "check" for s in scn.steps) and checks > 0
        assert ix.debug_get(_native.TM_DEBUG_PATH_SMALL) >= 2 * checks and ix.debug_get(_native.TM_DEBUG_PATH_PHASES) >= 2 * checks
    finally:
        ix.debug_set(_native.TM_DEBUG_PHASES, 0)
        ix.close()
