"""Device snapshots without a device: INFO_FIELDS are qs_snapshot_info's; EnvSnapshot files keep every bit; the digests
decide which snapshots an environment takes; and csrc/qs_snapshot.h -- the row's layout and the lane-level copies the kernels run -- moves
every float exactly once on the host, under AddressSanitizer and UBSan (a stand-alone program: tests/sanitize/drv_snapshot.cpp)."""
import os
import re
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_info_struct_matches_the_header():
    """INFO_FIELDS, the keys of a snapshot's header, are qs_snapshot_info's fields in the struct's order (the Structure against the header: test_abi_cpu.py)"""
    from qs_amd.snapshot import INFO_FIELDS, SnapshotInfo
    assert [n for n, _ in SnapshotInfo._fields_] == list(INFO_FIELDS) and list(SnapshotInfo().as_dict()) == list(INFO_FIELDS)


def _info(**kw):
    base = dict(bytes=3 * 352 * 4, n_envs=3, row_floats=352, rec_floats=288, push_floats=8, obs_dim=27, layout_version=1,
                layout_digest=0xfedcba9876543210, config_digest=0x8123456789abcdef)
    base.update(kw)
    return base


def test_files_keep_every_bit(tmp_path):
    """rows filled from random uint32 -- NaNs with payloads, negative zeros, denormals -- come back bit for bit, and so do the 64-bit digests
    and the arrays of extras, nested snapshot included"""
    import torch
    from qs_amd.snapshot import EnvSnapshot
    rng = np.random.default_rng(5)
    bits = rng.integers(0, 2 ** 32, size=(3, 352), dtype=np.uint64).astype(np.uint32)
    bits[0, :4] = [0x80000000, 0x7fc01234, 0xffc00001, 0x00000001]     # -0, two NaN payloads, a denormal
    inner = EnvSnapshot(torch.from_numpy(bits[:1].copy().view(np.float32)), _info(n_envs=1, bytes=352 * 4))
    extras = dict(vec_normalize=dict(stats=dict(obs_mean=rng.normal(size=27), obs_count=np.asarray(1e-4 + 40.0)), returns=torch.from_numpy(rng.normal(size=3)),
                                     old_reward=torch.from_numpy(bits[:, 0].copy().view(np.float32))),
                  rsi=dict(rng='{"state": 1}', counter=np.arange(3)), note="x", inner=inner, flags=[True, None, 2, 0.1])
    snap = EnvSnapshot(torch.from_numpy(bits.copy().view(np.float32)), _info(), extras)
    path = str(tmp_path / "snap.npz")
    snap.save(path)
    back = EnvSnapshot.load(path)
    assert back.rows.device.type == "cpu" and back.rows.dtype == torch.float32
    assert np.array_equal(back.rows.numpy().view(np.uint32), bits)
    assert back.info == snap.info and back.layout_digest == 0xfedcba9876543210 and back.config_digest == 0x8123456789abcdef and back.n_envs == 3
    x = back.extras["vec_normalize"]
    assert np.array_equal(x["stats"]["obs_mean"], extras["vec_normalize"]["stats"]["obs_mean"]) and x["stats"]["obs_mean"].dtype == np.float64
    assert float(x["stats"]["obs_count"]) == 1e-4 + 40.0
    assert np.array_equal(x["returns"], extras["vec_normalize"]["returns"].numpy()) and x["returns"].dtype == np.float64
    assert np.array_equal(np.asarray(x["old_reward"]).view(np.uint32), bits[:, 0])
    assert back.extras["rsi"]["rng"] == '{"state": 1}' and np.array_equal(back.extras["rsi"]["counter"], np.arange(3))
    assert back.extras["note"] == "x" and back.extras["flags"] == [True, None, 2, 0.1]
    assert np.array_equal(back.extras["inner"].rows.numpy().view(np.uint32), bits[:1]) and back.extras["inner"].n_envs == 1


def test_the_digests_decide_what_fits():
    from qs_amd.snapshot import check_fits, first_difference
    env = _info()
    check_fits(_info(), env, strict=True)
    with pytest.raises(ValueError, match="layout_digest"):
        check_fits(_info(layout_digest=1), env, strict=True)
    with pytest.raises(ValueError, match="layout_digest"):
        check_fits(_info(layout_digest=1), env, strict=False)
    with pytest.raises(ValueError, match="config_digest"):
        check_fits(_info(config_digest=2), env, strict=True)
    check_fits(_info(config_digest=2), env, strict=False)
    # the first differing field is the one named
    assert first_difference(_info(n_envs=4, obs_dim=28, layout_digest=1), env) == "n_envs"
    assert first_difference(_info(obs_dim=28, layout_digest=1), env) == "obs_dim"
    with pytest.raises(ValueError, match="n_envs is 4, the environment's is 3"):
        check_fits(_info(n_envs=4, layout_digest=1, config_digest=2), env, strict=False)


def test_a_saved_header_with_another_digest_is_refused_after_loading(tmp_path):
    """through a file: what load() hands back is what restore() compares"""
    import torch
    from qs_amd.snapshot import EnvSnapshot, check_fits
    path = str(tmp_path / "s.npz")
    EnvSnapshot(torch.zeros((3, 352)), _info(config_digest=77)).save(path)
    back = EnvSnapshot.load(path)
    with pytest.raises(ValueError, match="config_digest"):
        check_fits(back.info, _info(), strict=True)
    check_fits(back.info, _info(), strict=False)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("snap")
    exe = str(d / "drv_snapshot")
    subprocess.check_call(["g++", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-std=c++17", "-Wall",
                           "-Wno-unknown-pragmas", "-I" + os.path.join(REPO, "quadruped-springs_amd", "csrc"), "-o", exe,
                           os.path.join(REPO, "tests", "sanitize", "drv_snapshot.cpp")])
    return exe


@pytest.mark.parametrize("obs_dim", [27, 28, 1, 33, 64])     # PPO_BASIC's width; a multiple of 4; the smallest; pad 2; the widest (one wave)
def test_the_row_copies_on_the_host(driver, obs_dim):
    """snapshot -> scramble -> restore, a fork with a chain, one with a swap and one with a source out of range on fake records of three
    environments whose every float is its own bit pattern: every float of a row is covered exactly once, a fork changes everything but the
    two kept fields, chain and swap read pre-call values (the driver says what is wrong otherwise)"""
    r = subprocess.run([driver, str(obs_dim)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok")


def test_the_layout_is_stated_once():
    """the header states the row and the kept fields; the kernels and the host driver take both from it"""
    h = open(os.path.join(REPO, "quadruped-springs_amd", "csrc", "qs_snapshot.h")).read()
    assert "record: QS_REC | push row: PUSH_F | last observation: obs_dim | terminal observation: obs_dim" in h
    assert re.search(r"fork_keeps\(int rec_float\) \{ return rec_float == R_EPISODE \|\| rec_float == R_TOTAL_STEPS; \}", h)
    k = open(os.path.join(REPO, "quadruped-springs_amd", "csrc", "qs_snapshot.hip")).read()
    for name in ("k_snapshot", "k_restore", "k_fork_gather", "k_fork"):
        assert re.search(r"__global__[^\n]*\b%s\(" % name, k), name
    assert "__shared__" not in k
