"""One physics substep of every build of Sim ON THE GPU (tests/hip/substep_probe.hip: pyramid and cone, each the full and the common-path
build; cone common-path with the payload block's rows) against the float64 oracle and the host twin, on the case families of
tests/substep_cases.py (flight, stance, at the stops, fallen, the mass randomizer's parameters with pushes, wave edges):

  * full build: every group of quantities inside `FACTOR x max(own_i, P99 own)` of the float64 oracle (own = |oracle32 - oracle64|, per
    environment and per family; tests/test_substep_cpu.py holds the host twin to 0.7 of it) and inside the same bound of the host twin;
    contact flags, invalid-contact counts and substep's return value EQUAL to both;
  * common-path builds: the return value is the wave's vote over what the twin returns per environment; a wave that gives up hands state,
    warm start and payload block back bit for bit; a wave that finishes gives the full build's result bit for bit (the twin's two builds
    are bitwise equal on every finished row: checked here per row);
  * an environment gives the same bits alone among fifteen in flight as in a mixed wave, and results do not depend on the launch's size;
  * shapes the probe does not hold are refused with the outputs left NaN.

p50 / p90 / p99 / max of |device - oracle64| next to the oracle's own are printed and, where QS_RECORD_DIR names a directory, appended to
its substep_parity.jsonl (profiles/substep_parity.json is assembled from it): recorded, not asserted.

What runs here is the substep's source in a small kernel, not the code inlined into k_step / k_step_dense: the end-to-end parity tests
and tools/gate.sh stay the check for that."""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "hip"))
import substep_cases as SC  # noqa: E402
import substep_probe  # noqa: E402
from emu import emu as E  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the GPU box"
    return torch


def record(rec):
    """one line per case into $QS_RECORD_DIR/substep_parity.jsonl; nothing without the variable"""
    print(json.dumps(rec))
    out = os.environ.get("QS_RECORD_DIR")
    if out:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "substep_parity.jsonl"), "a") as f:
            f.write(json.dumps(rec) + "\n")


def device(c, build):
    rc, rec, ret, counters = substep_probe.substep(c.cfg, c.rec, c.tau, c.push, build)
    assert rc == 0, f"probe returned {rc}"
    assert not np.isnan(rec[:, SC.out_cols(c.cfg)]).any() and (ret >= 0).all(), "the kernel wrote every output"
    keep = np.setdiff1d(np.arange(rec.shape[1]), np.r_[SC.out_cols(c.cfg), 219:243])       # (219..242: the torque slots store_state writes back)
    assert np.array_equal(rec[:, keep].view(np.uint32), c.rec[:, keep].view(np.uint32)), "the substep writes its outputs only"
    return rec, ret, counters


def check_case(c, label):
    """every build of the case's configuration on the device; -> the record line"""
    twin_full, _ = E.substep(c.cfg, c.rec, c.tau, c.push, "full")
    dev_full, ret, counters = device(c, "full")
    assert (ret == 0).all(), "the full build returns 0"
    got, twin = SC.from_records(c.cfg, dev_full), SC.from_records(c.cfg, twin_full)
    r64 = SC.check_against_oracle(c, got, f"device full {label}")
    rtw = SC.ratios(c, got, ref=twin)
    bad = {g: v for g, v in rtw.items() if v[0] > 1.0}
    assert not bad, f"device full {label} against the host twin: group -> (|device - twin| / bound, environment, |d|, bound) {bad}"
    assert np.array_equal(got["foot_contact"], twin["foot_contact"]) and np.array_equal(got["n_invalid"], twin["n_invalid"]), f"{label}: flags against the twin"
    out = dict(case=label, n=int(c.kept), rejected=int(c.rejected), ratio_to_bound={g: round(v[0], 3) for g, v in r64.items()},
               ratio_to_bound_against_twin={g: round(v[0], 3) for g, v in rtw.items()}, quantiles_p50_p90_p99_max=SC.quantiles(c, got),
               many_rows_wave_substeps=int(counters[0]), self_narrow_wave_substeps=int(counters[1]), builds={})
    oc = SC.out_cols(c.cfg)
    for build in SC.builds_of(c.config_name)[1:]:
        twin_hot, twin_ret = E.substep(c.cfg, c.rec, c.tau, c.push, build)
        same = (SC.bits(twin_hot[:, oc]) == SC.bits(twin_full[:, oc])).all(axis=1)      # the twin's two builds, per row
        dev_hot, dev_ret, _ = device(c, build)
        out["builds"][build] = SC.check_common_path(c, dev_hot, dev_ret, dev_full, SC.fold_waves(twin_ret), same, f"device {build} {label}")
    return out, dev_full, counters


@pytest.mark.parametrize("family,config", SC.MATRIX)
def test_device_substep(torch_cuda, family, config):
    c = SC.family(family, config)
    assert c.rejected <= SC.CAP * c.draws and c.kept == SC.N_FAMILY
    out, _, counters = check_case(c, f"{family} / {config}")
    if family == "stops":
        assert counters[0] == c.kept // 16, "every wave of the full build ran the many-rows solve (the limit rows)"
        assert all(b["gave_up"] == c.kept for b in out["builds"].values())
    if family == "fallen":
        assert counters[0] >= c.kept // 32
    if family == "stance":      # the common path: no many-rows solve, and the build that holds the handle's rows finishes
        assert counters[0] == 0 and out["builds"][SC.builds_of(config)[-1]]["finished"] == c.kept
    record(out)


@pytest.mark.parametrize("config", [c for _, c in SC.EDGES])
def test_wave_edges_and_independence(torch_cuda, config):
    c = SC.edges(config)
    out, dev_full, _ = check_case(c, f"edges / {config}")
    oc = SC.out_cols(c.cfg)
    for a, b in c.twice:        # alone among fifteen in flight, and in the mixed wave
        assert np.array_equal(c.rec[a].view(np.uint32), c.rec[b].view(np.uint32))       # (bit patterns: a record holds a NaN sentinel)
        assert np.array_equal(SC.bits(dev_full[a, oc]), SC.bits(dev_full[b, oc])), f"environment {a} against its copy {b} in the mixed wave"
    hot = SC.builds_of(config)[-1]
    assert out["builds"][hot]["finished"] >= 16 and out["builds"][hot]["gave_up"] >= 16, "wave 0 stays on the common path, the mixed wave gives up"
    # the launch's size: each wave alone
    for build in SC.builds_of(config):
        whole, whole_ret, _ = device(c, build)
        for w in range(3):
            sl = slice(16 * w, 16 * w + 16)
            rc, rec, ret, _ = substep_probe.substep(SC.config(config, 16), c.rec[sl], c.tau[sl], None if c.push is None else c.push[sl], build)
            assert rc == 0
            assert np.array_equal(SC.bits(rec[:, oc]), SC.bits(whole[sl][:, oc])) and np.array_equal(ret, whole_ret[sl]), f"{build}: wave {w} alone against the launch of 48"
    record(out)


def test_shapes_the_probe_does_not_hold_are_refused(torch_cuda):
    c = SC.edges("cone")
    rc, rec, ret, _ = substep_probe.substep(c.cfg, c.rec[:8], c.tau[:8], None, "full")          # not a whole wave
    assert rc == substep_probe.ERR_ARGS and np.isnan(rec).all() and (ret == -1).all()
    rc, rec, ret, _ = substep_probe.substep(c.cfg, c.rec[:16, :100], c.tau[:16], None, "full")  # not records
    assert rc == substep_probe.ERR_ARGS and np.isnan(rec).all()
    rc, rec, ret, _ = substep_probe.substep(c.cfg, c.rec[:16], c.tau[:16], None, "hot_soft")    # no payload block in this configuration
    assert rc == substep_probe.ERR_ARGS and np.isnan(rec).all() and (ret == -1).all()
    rc, rec, ret, _ = substep_probe.substep(SC.config("pyramid", 16), c.rec[:16], c.tau[:16], None, "hot_soft")
    assert rc == substep_probe.ERR_ARGS and np.isnan(rec).all()
