"""One physics substep of the kernel arithmetic on the HOST (tests/emu/qs_emu_substep.cpp: every build of Sim that tests/hip/substep_probe.hip
holds) against the float64 oracle, on the case families of tests/substep_cases.py -- the CPU side of tests/test_gpu_substep.py:

  * the margins reject at most 5 % of a family's draws (a condition on the generators);
  * the twin's full build sits inside `FACTOR x max(own_i, P99 own)` of the float64 oracle in every group (own = |oracle32 - oracle64|),
    with equal contact flags and invalid-contact counts -- and at or under TWIN_RATIO of it, which is what lets the GPU test hold the
    device to the whole bound;
  * the twin's common-path builds: they give up where the family says so, leave the state alone when they do, and match the full build
    where they do not;
  * the probe cross-compiles for gfx950."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "hip"))
import substep_cases as SC  # noqa: E402
from emu import emu as E  # noqa: E402

# (family, configuration) -> the twin's worst ratio where it is above TWIN_RATIO, as measured: none
ABOVE = {}


def test_layout_constants():
    e = E.Emu(SC.config("cone", 1))
    for name in ("R_PARAMS", "R_POS", "R_WARM", "R_N_INVALID", "R_FOOT_FORCE", "R_FOOT_CONTACT", "R_BLOCK"):
        assert e.field(name) == getattr(SC, name), name


@pytest.mark.parametrize("family,config", SC.MATRIX)
def test_cap_and_twin_against_the_oracles(family, config):
    c = SC.family(family, config)
    assert c.rejected <= SC.CAP * c.draws and c.kept == SC.N_FAMILY, f"{c.rejected} of {c.draws} draws rejected: {c.rejected_by}"
    rec, ret = E.substep(c.cfg, c.rec, c.tau, c.push, "full")
    assert (ret == 0).all()
    r = SC.check_against_oracle(c, SC.from_records(c.cfg, rec), f"twin {family} / {config}")
    worst = max(v[0] for v in r.values())
    print(f"{family} / {config}: rejected {c.rejected_by}; twin's worst ratio {worst:.2f}: { {g: round(v[0], 2) for g, v in r.items()} }")
    assert worst <= ABOVE.get((family, config), SC.TWIN_RATIO) + 0.005, f"the twin's worst |twin - oracle64| / bound is {worst:.2f}"
    # the float32 oracle is inside the bound by construction (FACTOR > 1): the bound is not degenerate
    assert all(v[0] <= 1.0 / SC.Y.FACTOR + 1e-12 for v in SC.ratios(c, c.o32).values())
    if family == "flight":
        assert not c.o64["foot_contact"].any() and (np.abs(c.states[:, 25:37]) > c.cfg.vel_cap).any()
    if family == "stance":
        assert set(c.o64["foot_contact"].sum(axis=1).astype(int)) == {0, 1, 2, 3, 4}
    if family == "stops":
        assert (ret == 0).all() and ((c.states[:, 13:25] < SC.JLO) | (c.states[:, 13:25] > SC.JHI)).any(axis=1).all()
    if family == "fallen":
        assert (c.o64["n_invalid"] > 0).sum() >= SC.N_FAMILY // 2
    if family == "parameters":
        assert (c.push[:, 6] > 0).sum() >= 64 and set(c.push[c.push[:, 6] > 0, 7]) == {1.0, 2.0} and (c.params[:, SC.P_M_PAY] > 0).all()


@pytest.mark.parametrize("family,config", SC.MATRIX + SC.EDGES)
def test_twin_common_path_builds(family, config):
    c = SC.edges(config) if family == "edges" else SC.family(family, config)
    full, _ = E.substep(c.cfg, c.rec, c.tau, c.push, "full")
    for build in SC.builds_of(config)[1:]:
        rec, ret = E.substep(c.cfg, c.rec, c.tau, c.push, build)
        if family == "stops" or (build == "hot" and c.cfg.payload_soft):
            assert (ret == 1).all(), "the common-path build gives up at a stop, and on every substep of a handle with the payload block"
        if family == "flight" and not c.cfg.self_collision:
            assert (ret == 0).all()
        oc = SC.out_cols(c.cfg)
        same = (SC.bits(rec[:, oc]) == SC.bits(full[:, oc])).all(axis=1)
        out = SC.check_common_path(c, rec, ret, full, ret, same, f"twin {build} {family} / {config}")
        print(f"{family} / {config} {build}: {out}")


def test_probe_builds_for_gfx950():
    """the probe cross-compiles with the product's options and exports its entry point"""
    import substep_probe
    so = substep_probe.build()
    syms = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    assert "qsp_substep" in syms
    with open(so, "rb") as f:
        assert b"gfx950" in f.read()
