"""tests/norm_ref.py judged without a GPU, so that tests/test_gpu_norm_shapes.py can neither hide a failure nor fail on the reference's
account: the float64 reference's batch moments lie within a tenth of the device tolerances of exact (np.longdouble) ones in every step of
every case; every mask has the property its name claims at the handle's own rows_per_block; the shape list reaches the part counts it is
there for; both clip edges saturate."""
import numpy as np
import pytest

import norm_ref as R

CASES = [(n, o, False) for n, o in dict.fromkeys(R.SHAPES + R.FLAG_SHAPES)] + [(n, o, True) for n, o in R.MASK_SHAPES]


def test_longdouble_is_wider_than_float64():
    assert np.finfo(np.longdouble).eps < 1e-18, "np.longdouble is float64 here: the reference cannot be judged on this machine"


@pytest.mark.parametrize("n, o, masked", CASES)
def test_reference_moments_against_longdouble(n, o, masked):
    worst = dict(mean=0.0, var=0.0, ret_mean=0.0, ret_var=0.0)
    edges = dict(lo=0, hi=0, term_lo=0, term_hi=0)
    batches = []

    def look(k, ref, step, exp):
        for key, arr in (("", exp["obs"]), ("term_", exp.get("term"))):
            if arr is not None:
                edges[key + "lo"] += int((arr == -R.CLIP_OBS).sum()); edges[key + "hi"] += int((arr == R.CLIP_OBS).sum())
        if k < 0 or not step["training"]:
            return
        b = ref.batch
        batches.append(len(b["returns"]))
        if not len(b["returns"]):
            return
        x = np.asarray(b["obs"], np.float64)                  # RunningMeanStd.update(moments_dtype=np.float64)
        m64, v64 = np.mean(x, axis=0), np.var(x, axis=0)
        m, v = R.exact_moments(x)
        bound = R.MEAN_REL * np.abs(m) + R.MEAN_STD * np.sqrt(v)
        assert (np.abs(m64 - m) <= 0.1 * bound).all(), (k, np.max(np.abs(m64 - m) / np.where(bound > 0, bound, 1)))
        assert (np.abs(v64 - v) <= 0.1 * R.VAR_RTOL * v).all(), (k, np.max(np.abs(v64 - v) / np.where(v > 0, v, 1)))
        worst["mean"] = max(worst["mean"], float(np.max(np.where(bound > 0, np.abs(m64 - m) / np.where(bound > 0, bound, 1), 0))))
        worst["var"] = max(worst["var"], float(np.max(np.where(v > 0, np.abs(v64 - v) / np.where(v > 0, v, 1), 0)) / R.VAR_RTOL))
        r = b["returns"]
        rm, rv = R.exact_moments(r)
        for name, got, want in (("ret_mean", np.mean(r), rm), ("ret_var", np.var(r), rv)):
            bound = R.MOM_RTOL * abs(want) + R.MOM_ATOL
            assert abs(got - want) <= 0.1 * bound, (k, name, float(abs(got - want) / bound))
            worst[name] = max(worst[name], float(abs(got - want) / bound))

    R.run_reference(n, o, masked=masked, on_step=look)
    print(f"reference against longdouble, ratio to the device bounds ({n}, {o}, masked={masked}):", worst, "saturated:", edges)
    assert len(batches) == R.TRAIN_STEPS
    if n >= 64 and o >= R.KINDS:     # (a width that has a column of the sixth kind; in a batch of n rows no value lies further than sqrt(n) of its own
        #                              standard deviations from the mean: below 64 rows the two planted ones widen the statistics instead)
        assert min(edges.values()) >= 1, edges
    if masked:
        on = [int(m.sum()) for m in R.masks(n, np.random.default_rng(R.seed_of(n, o, 77)))]
        assert batches == on and batches[3] == 0 and batches[2] == 1 and batches[5] == n


@pytest.mark.parametrize("n, o", R.MASK_SHAPES)
def test_masks_are_what_their_names_claim(n, o):
    rows, parts = R.layout(n)
    assert parts > 2
    m = dict(zip(R.MASKS, R.masks(n, np.random.default_rng(R.seed_of(n, o, 77)))))
    assert all(x.dtype == np.uint8 and x.shape == (n,) and set(np.unique(x)) <= {0, 1} for x in m.values())
    per_block = lambda x: [int(x[b * rows:(b + 1) * rows].sum()) for b in range(parts)]
    a = per_block(m["rows_0_100_off"])
    assert a[0] == 0 and 0 < a[1] < rows and not m["rows_0_100_off"][:100].any() and m["rows_0_100_off"][100:].all()     # block 0 empty, block 1 partly counted
    b = per_block(m["middle_block_and_first_rows_off"])
    mid = parts // 2
    assert 0 < mid < parts - 1 and b[mid] == 0 and b[0] > 0 and all(x > 0 for i, x in enumerate(b[:-1]) if i != mid)
    assert not m["middle_block_and_first_rows_off"][::rows].any()
    assert per_block(m["only_last_row"]) == [0] * (parts - 1) + [1] and m["only_last_row"][n - 1] == 1
    assert not m["none"].any() and m["ones"].all()
    e = m["random_60"]
    assert 0.5 < e.mean() < 0.7 and min(per_block(e)[:-1]) > 0 and 0 < e[::rows].sum() < parts      # counted and uncounted first rows of a block
    seq = R.sequence(n, o, masked=True)
    assert [s["training"] for s in seq] == [1] * R.TRAIN_STEPS + [0] * R.EVAL_STEPS and all(s["active"] is None for s in seq[R.TRAIN_STEPS:])
    for k, name in enumerate(R.MASKS):
        s = seq[k]
        assert np.array_equal(s["active"], m[name])
        off = s["active"] == 0
        if off.any() and k != 4:
            assert s["done"][off].any(), f"{name}: no uncounted row ends an episode"     # a return that must not clear
    assert seq[2]["done"].all() and not seq[4]["done"].any()
    planted = seq[1]["obs"][::rows, 0::R.KINDS]
    assert (planted == R.PLANTED).all() and np.abs(seq[1]["obs"][1::rows, 0]).max() < 10


def test_shapes_reach_the_part_counts():
    assert R.layout(200) == (64, 4) and 200 - 3 * 64 == 8
    assert R.layout(1)[1] == R.layout(7)[1] == R.layout(9)[1] == R.layout(64)[1] == 1 and R.layout(65)[1] == 2
    assert R.layout(513) == (64, 9)                 # lane group ry = 0 of k_norm_finish merges two parts
    assert R.layout(4097) == (64, 65)               # 65 parts: the second pass of the merge loop (8 lane groups x QN_MCH = 8 parts per pass)
    rows, parts = R.layout(32769)
    assert (rows, parts) == (72, 456) and rows % 32 != 0 and 32769 - (parts - 1) * rows == 9
    assert all(R.layout(n)[1] <= R.QN_MAX_PARTS for n in (32769, 65536, 1 << 20))
    assert sorted({o + 1 for _, o in R.WIDTHS}) == [2, 32, 33, 34, 64, 65, 66, 256]
    assert {n for n, _ in R.SIZES} == {1, 7, 9, 64, 65, 513, 4097, 32769} and (4097, 255) in R.SHAPES
    assert max(n * o for n, o in R.SHAPES) == 32769 * 33 < 1.04 * 4097 * 255       # the largest arrays: 4.3 MB and 4.2 MB of float32


def test_data_is_what_the_table_says():
    n, o = 4097, 65
    seq = R.sequence(n, o)
    x = np.concatenate([s["obs"] for s in seq]).astype(np.float64)
    assert x.dtype == np.float64 and seq[0]["obs"].dtype == np.float32
    for c in range(12):
        mean, var = R.NOMINAL[c % R.KINDS]
        col = x[:, c]
        if c % R.KINDS == 2:
            assert (col == mean).all()
        elif c % R.KINDS == 4:
            assert set(np.unique(col)) == {0.0, 1.0} and 0.005 < col.mean() < 0.015
        else:
            assert abs(col.mean() - mean) < 0.05 * np.sqrt(var) and 0.9 * var < col.var() < 1.1 * var, c
    assert abs(np.mean([s["done"].mean() for k, s in enumerate(seq) if k not in (2, 4)]) - 0.02) < 0.005
    rew = R.sequence(*R.OFFSET_REWARDS)[0]["rew"]
    assert abs(rew.mean() - 1000.0) < 0.01 and 0.005 < rew.std() < 0.02
    again = R.sequence(n, o)
    assert all(np.array_equal(a[k], b[k]) for a, b in zip(seq, again) for k in ("obs", "term", "rew", "done"))


@pytest.mark.parametrize("flags", R.FLAGS)
def test_reference_flags(flags):
    """what the GPU file asks of the kernels under norm_obs = 0 and training = 0 holds in the reference"""
    training, norm_obs, norm_reward = flags
    n, o = R.FLAG_SHAPES[0]
    seen = []

    def look(k, ref, step, exp):
        seen.append((k, {key: np.copy(v) for key, v in ref.stats().items()}, ref.returns.copy()))
        if not norm_obs:
            assert np.array_equal(exp["obs"], step["obs"]) and (k < 0 or np.array_equal(exp["term"], step["term"]))
        if k >= 0 and not norm_reward:
            assert np.array_equal(exp["rew"], step["rew"])

    R.run_reference(n, o, flags=flags, on_step=look)
    first, last = seen[1][1], seen[-1][1]
    moved = lambda key: not np.array_equal(first[key], last[key])
    assert moved("ret_var") == moved("ret_count") == bool(training)
    assert moved("obs_mean") == moved("obs_count") == bool(training and norm_obs)
