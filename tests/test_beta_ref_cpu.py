"""tests/beta_ref.py judged before any kernel is judged by it (no GPU): the fp64 restatement against the
LibTorch golden and the C oracle, the constants K_REF of its bound measured on the reference's own fp32
arithmetic, the sampler's moment bounds on the oracle's sampler, and the update cases' distance from the clip
edges."""
import numpy as np
import pytest

import beta_ref as B
import oracle_lib as Orc
from golden_io import load_case

SHAPES = [(17, 6, 64), (11, 3, 64), (17, 17, 64)]   # the oracle's arithmetic does not depend on the width


def _biases(load):
    return (np.array([B.bias_of(t[0]) for t in load], np.float32), np.array([B.bias_of(t[1]) for t in load], np.float32))


def same_nonfinite(dev, ref):
    """-inf where the reference is -inf, NaN where it is NaN, finite where it is finite"""
    dev, ref = np.asarray(dev, np.float64), np.asarray(ref, np.float64)
    return (np.array_equal(np.isnan(dev), np.isnan(ref)) and np.array_equal(np.isneginf(dev), np.isneginf(ref))
            and np.array_equal(np.isposinf(dev), np.isposinf(ref)))


def test_fp64_restatement_reproduces_the_libtorch_golden():
    """beta_dist: 256 concentrations in [1, 8], x in [0.01, 0.99]; the bar test_oracle_golden.py holds the
    oracle's formulas to (rtol 2e-5, atol 2e-5), and the mean at rtol 1e-6."""
    _, d = load_case("beta_dist")
    r = B.beta_fp64(d["alpha"], d["beta"], d["x"])
    np.testing.assert_allclose(r["lp"].numpy(), d["log_prob"], rtol=2e-5, atol=2e-5)
    np.testing.assert_allclose(r["ent"].numpy(), d["entropy"], rtol=2e-5, atol=2e-5)
    np.testing.assert_allclose(r["mean"].numpy(), d["mean"], rtol=1e-6, atol=0)


def test_head_params_hit_their_targets():
    """The biases give the grid's concentrations: 1 exactly, the thresholds exactly where an fp32 bias can
    (3, 6 and its predecessor, 10, 21 at pre-activation 20, and the identity range)."""
    L = Orc.layout_init(1, 17, 6, 64)
    tg = [1.0, 3.0, 5.9999995, 6.0, 10.0, 21.0]
    p, al, be = B.head_params(L, np.random.default_rng(0), tg, [22.0, 100.0, 1000.0, B.Bias(-15.0), 1.05, 9.5])
    np.testing.assert_array_equal(al, np.array(tg, np.float32))
    np.testing.assert_array_equal(be[:3], np.array([22, 100, 1000], np.float32))
    assert 1 < be[3] < 1 + 1e-6 and abs(be[4] - 1.05) < 1e-6 and abs(be[5] - 9.5) < 1e-6
    assert not p[L.aW3:L.aW3 + 6 * 64].any() and not p[L.bW3:L.bW3 + 6 * 64].any()
    assert p[L.ab3] == -100.0 and p[L.ab3 + 5] == 20.0 and p[L.bb3 + 2] == 999.0


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "O%d_A%d_H%d" % s)
def test_fp64_restatement_agrees_with_the_oracle_forward(shape):
    """oracle_lib.get_action_and_value with given actions over the whole grid and the far point: log-prob
    and entropy within the bound at factor 1; -inf at action = hi with beta > 1 and NaN above hi (the clamp
    lets s = 1 + 2^-23 through, so log(1 - s) is NaN: the reference's own behaviour) in the same rows."""
    O_, A, H = shape
    L = Orc.layout_init(1, O_, A, H)
    rng = np.random.default_rng(1)
    worst = {"lp": 0.0, "ent": 0.0}
    for load in B.grid_loads(A) + [[B.FAR] * A]:
        p, al, be = B.head_params(L, rng, [t[0] for t in load], [t[1] for t in load])
        act, names = B.given_actions(al, be, 10)
        x = rng.standard_normal((10, O_)).astype(np.float32)
        _, lp, ent, _ = Orc.get_action_and_value(L, p, x, 1, act)
        ref = B.beta_fp64(np.broadcast_to(al, act.shape), np.broadcast_to(be, act.shape), B.scale_action(act))
        rl, re_ = ref["lp"].numpy().sum(-1), ref["ent"].numpy().sum(-1)
        bd = B.row_bounds(ref, factor=1.0)
        assert same_nonfinite(lp, rl), (names, lp, rl)
        ok = np.isfinite(rl)
        assert np.isfinite(re_).all() and np.isfinite(ent).all()
        with np.errstate(invalid="ignore"):
            el, ee = np.abs(lp - rl)[ok] / bd["lp"][ok], np.abs(ent - re_) / bd["ent"]
        worst["lp"], worst["ent"] = max(worst["lp"], el.max()), max(worst["ent"], ee.max())
        assert (el <= 1).all() and (ee <= 1).all(), (load, el.max(), ee.max())
    print("oracle forward, largest error / bound:", worst)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "O%d_A%d_H%d" % s)
@pytest.mark.parametrize("setting", ["logp", "ent", "default"])
def test_fp64_restatement_agrees_with_the_oracle_gradient(shape, setting):
    """oracle_lib.minibatch_grad's head-bias gradients on the update cases of every grid load, element by
    element within the bound at factor 1; its loss statistics within theirs."""
    O_, A, H = shape
    M, clip = 111, 0.2
    L = Orc.layout_init(1, O_, A, H)
    rng = np.random.default_rng(2)
    ent_coef = {"logp": 0.0, "ent": 1.0, "default": 0.01}[setting]
    worst = 0.0
    for load in B.grid_loads(A):
        p, al, be = B.head_params(L, rng, [t[0] for t in load], [t[1] for t in load])
        act, ref, old, adv = B.update_case(al, be, M, rng)
        if setting == "ent":
            adv = np.zeros_like(adv)
        x = rng.standard_normal((M, O_)).astype(np.float32)
        ret, ov = rng.standard_normal(M).astype(np.float32), rng.standard_normal(M).astype(np.float32)
        g, st = Orc.minibatch_grad(L, p, x, act, old, adv, ret, ov, Orc.LossCfg(clip, ent_coef, 0.5, 1, 0))
        u = B.update_fp64(ref, old, adv, clip, ent_coef, p[L.ab3:L.ab3 + A], p[L.bb3:L.bb3 + A], factor=1.0)
        for h, off in (("a", L.ab3), ("b", L.bb3)):
            r = np.abs(g[off:off + A] - u["g" + h]) / u["g" + h + "_bound"]
            worst = max(worst, r.max())
            assert (r <= 1).all(), (load, h, r)
        for k, i in (("pg_loss", 0), ("entropy", 2), ("old_approx_kl", 3), ("approx_kl", 4), ("clipfrac", 5)):
            assert abs(st[i] - u["stats"][k]) <= u["stats_bound"][k] + 1e-7 * abs(u["stats"][k]), (load, k)
    print(f"oracle head-bias gradient ({setting}), largest error / bound: {worst:.3f}")


def _grid_items():
    al, be, s = [], [], []
    for ta, tb in B.grid_pairs():
        a, b = B.conc_of_bias(B.bias_of(ta)), B.conc_of_bias(B.bias_of(tb))
        act, _ = B.given_actions(np.array([a]), np.array([b]), len(B.GIVEN))
        for si in B.scale_action(act)[:, 0]:
            al.append(a); be.append(b); s.append(si)
    return np.array(al, np.float32), np.array(be, np.float32), np.array(s, np.float32)


def _dense_items(per_decade=40000):
    rng = np.random.default_rng(0)
    n = 3 * per_decade
    return ((10 ** rng.uniform(0, 3, n)).astype(np.float32), (10 ** rng.uniform(0, 3, n)).astype(np.float32),
            rng.uniform(1e-3, 1 - 1e-3, n).astype(np.float32))


def test_reference_fp32_arithmetic_measures_k_ref():
    """The reference's formulas in torch float32 on the CPU (gradients by autograd) against beta_fp64 on
    every given-action item of the grid and on 40 000 log-uniform (alpha, beta) per decade of [1, 1000]:
    the largest |error| / (2^-24 sum |addends|) of each quantity is at most its K_REF. This is where K_REF
    comes from (beta_ref.py); no kernel's result enters. The fp32 arithmetic is non-finite exactly where
    the restatement is."""
    meas = {k: 0.0 for k in B.K_REF}
    for al, be, s in (_grid_items(), _dense_items()):
        ref, f32 = B.beta_fp64(al, be, s), B.beta_torch_fp32(al, be, s)
        for q, keys in (("lp", ["lp"]), ("ent", ["ent"]), ("dlp", ["dlp_da", "dlp_db"]), ("dent", ["dent_da", "dent_db"])):
            for k in keys:
                r, m, f = ref[k].numpy(), ref["mag_" + k].numpy(), f32[k].double().numpy()
                assert same_nonfinite(f, r), k
                ok = np.isfinite(r) & np.isfinite(m)
                err = np.abs(f[ok] - r[ok])
                sel = err > (B.FLOOR_ITEM if q in ("lp", "ent") else 0.0)
                if sel.any():
                    meas[q] = max(meas[q], float((err[sel] / (B.U * m[ok][sel])).max()))
    print("measured K (torch fp32 on the CPU):", {k: round(v, 3) for k, v in meas.items()}, "K_REF:", B.K_REF)
    for k in B.K_REF:
        assert 0 < meas[k] <= B.K_REF[k], (k, meas[k])
        assert B.K_REF[k] <= 1.5 * meas[k], (k, meas[k])   # the recorded constant stays a measurement


def test_oracle_sampler_passes_the_moment_bounds():
    """The oracle's Marsaglia-Tsang Beta sampler at the Philox counters of a 37-env, 32-step rollout
    (iteration 0) passes the 5-sigma bounds on its first three moments at every grid pair, and every sample
    lies in [FLT_MIN, 1 - 2^-24]: the bounds hold for a correct sampler."""
    worst = np.zeros(3)
    for i, (ta, tb) in enumerate(B.grid_pairs()):
        al, be = B.conc_of_bias(B.bias_of(ta)), B.conc_of_bias(B.bias_of(tb))
        s = B.oracle_samples(al, be, i % 6, 37, 32)
        assert s.min() >= B.FLT_MIN and s.max() <= B.S_MAX
        r = np.array(B.moment_check(s.ravel(), al, be))
        assert (r < 1).all(), (float(al), float(be), r)
        worst = np.maximum(worst, r)
    print("oracle sampler, largest |deviation| / (5 sd) of mean, variance, third moment:", worst.round(3))


def test_central_moments_are_exact():
    """Beta(2, 3): mean 2/5, variance 1/25, third central moment 2/875 (closed forms)."""
    mu, m = B.beta_central_moments(2.0, 3.0)
    np.testing.assert_allclose([mu, m[2], m[3]], [0.4, 0.04, 2.0 * 2 * 3 * (3 - 2) / (5 ** 3 * 6 * 7)], rtol=1e-14)
    _, m = B.beta_central_moments(1000.0, 1.0)
    assert 0 < m[6] < 1e-15   # beyond fp64 from raw moments: 15 sigma^6 ~ 1e-17


@pytest.mark.parametrize("A", [3, 6, 8, 17])
def test_update_cases_keep_clear_of_the_clip_edges(A):
    """No row's fp64 ratio lies within its log-prob bound of 1 +- clip_coef: the excluded set is empty, so
    clipfrac and the clipped / unclipped branch of every row are the same in fp64 and in any copy within
    its bound. Both branches and both advantage signs occur."""
    rng = np.random.default_rng(3)
    for load in B.grid_loads(A):
        ba, bb = _biases(load)
        al, be = B.conc_of_bias(ba), B.conc_of_bias(bb)
        act, ref, old, adv = B.update_case(al, be, 111, rng)
        u = B.update_fp64(ref, old, adv, 0.2, 0.01, ba, bb)
        assert np.isfinite(u["lp_bound"]).all() and u["edge_margin"].min() > 1, (load, u["edge_margin"].min())
        assert 0.2 < u["stats"]["clipfrac"] < 0.8 and (adv > 0).any() and (adv < 0).any()
        assert np.isfinite(u["ga"]).all() and np.isfinite(u["gb"]).all()
