"""The Beta policy head restated once in float64, the grid of concentrations its kernel copies are judged
on, and the bound they are judged by (test_beta_ref_cpu.py, test_gpu_beta_range.py). No GPU here.

The head (rl_utils.h:48-132; ac:194-249): alpha, beta = softplus(pre) + 1 per action dimension, a sample or
a given action scaled to s in [0, 1], log-prob and entropy summed over the A dimensions of a row.

The bound. A kernel copy holds fp32 concentrations and an fp32 s and evaluates sums whose addends are far
larger than the result at high concentration (lgamma(a + b) - lgamma(a) - lgamma(b) cancels to a few
units out of thousands), so a flat tolerance cannot hold over the range. Per row, for log-prob and entropy:

    bound = 5e-5                                           the project's bar against the LibTorch golden
          + f * K_REF * 2^-24 * sum_items mag              rounding of the addends: mag = sum |addend|
          + f * sum_items (|d/da| ulp(a) + |d/db| ulp(b))  the device's softplus may round a, b differently
          + sum_items |d lp/d s| ulp(action) / (hi - lo)   stored samples only: the action round trip

f = 2 for a kernel (v_rcp_f32 in place of IEEE division, another Stirling shift), f = 1 for the oracle.
K_REF is what the reference's own fp32 arithmetic (the same formulas in torch float32 on the CPU, gradients
by autograd) measures against beta_fp64 on the grid below: test_beta_ref_cpu.py measures it, prints it and
asserts it is at most the constant recorded here. It is not fitted to any kernel's result."""
from fractions import Fraction

import numpy as np
import torch

import oracle_lib as Orc

U = 2.0 ** -24          # fp32 unit roundoff
FLOOR = 5e-5            # tests/test_gpu_parity.py: log-prob / entropy against the LibTorch golden
FLT_MIN = float(np.finfo(np.float32).tiny)
S_MAX = float(np.float32(1) - np.float32(2.0 ** -24))   # the largest sample, nextafter(1, 0)
LO, HI = -1.0, 1.0

# max of |torch fp32 - fp64| / (2^-24 * sum |addends|) per item, measured on the CPU over the grid's items
# and 40 000 log-uniform (alpha, beta) per decade of [1, 1000] (a maximum over 48 pairs alone would
# understate the constant). For log-prob and entropy an item whose error is under FLOOR / 20 is left to
# the floor: at most 20 action dimensions are accepted, so such items cannot exceed the row's floor together.
# test_beta_ref_cpu.py::test_reference_fp32_arithmetic_measures_k_ref prints the measurement (logp 2.00,
# entropy 2.08, dlogp 11.8, dent 1.13) and asserts it is at most these; the headroom is for torch's
# vectorised special functions, which differ between CPUs.
K_REF = {"lp": 2.5, "ent": 2.6, "dlp": 13.0, "dent": 1.5}
FLOOR_ITEM = FLOOR / 20


class Bias:
    """A grid concentration given by its head bias instead of its value."""

    def __init__(self, b):
        self.b = float(b)


# concentrations of the grid (ISSUE: 1 exactly; bias -15; the thresholds x < 6 of the Stirling shift, x < 10
# and x == 10 of ATen's digamma (3.0: its shifts land on 10.0), softplus's 20; a trained policy's 100, 1000)
CONC = [1.0, Bias(-15.0), 1.05, 1.5, 2.0, 3.0, 5.9999995, 6.0, 9.5, 10.0, 21.0, 22.0, 100.0, 1000.0]
FAR = (1e4, 1e4)   # finiteness and the bound only: the reference's own fp32 formula is 2e-2 off there


def grid_pairs():
    """(alpha, beta) targets: symmetric, the most skewed both ways, (c, c / 10), and the pairs whose sum
    sits on the shift threshold 6."""
    pairs = [(c, c) for c in CONC]
    pairs += [(c, 1.0) for c in CONC[1:]] + [(1.0, c) for c in CONC[1:]]
    pairs += [(c, c / 10.0) for c in (21.0, 22.0, 100.0, 1000.0)]
    pairs += [(5.0, 1.0), (4.9999995, 1.0), (1.0, 5.0), (2.9999998, 3.0)]
    return pairs


def grid_loads(A):
    """The grid pairs in groups of A (one parameter load each); the last group is filled from the start."""
    pairs = grid_pairs()
    out = []
    for i in range(0, len(pairs), A):
        g = pairs[i:i + A]
        g += pairs[:A - len(g)]
        out.append(g)
    return out


def _softplus64(b):
    b = np.asarray(b, np.float64)
    return np.where(b > 20.0, b, np.log1p(np.exp(np.minimum(b, 20.0))))


def conc_of_bias(b32):
    """float32(softplus(bias)) + 1 in fp32: the concentration the reference forms from an fp32 bias."""
    return (_softplus64(np.asarray(b32, np.float32)).astype(np.float32) + np.float32(1.0)).astype(np.float32)


def bias_of(target):
    """The fp32 head bias of a target concentration: -100 for exactly 1 (softplus underflows), target - 1
    above 21 (softplus is the identity above 20), the inverse softplus otherwise, moved by a few ulps where
    that lands the reference's concentration on the fp32 target exactly."""
    if isinstance(target, Bias):
        return np.float32(target.b)
    t = np.float32(target)
    if t == np.float32(1.0):
        return np.float32(-100.0)
    if t > np.float32(21.0):
        return np.float32(t - np.float32(1.0))
    y = float(t) - 1.0
    b0 = np.float32(y + np.log(-np.expm1(-y)))
    cands = [b0]
    up = dn = b0
    for _ in range(8):
        up = np.nextafter(up, np.float32(np.inf)); dn = np.nextafter(dn, np.float32(-np.inf))
        cands += [up, dn]
    for b in cands:
        if conc_of_bias(b) == t:
            return np.float32(b)
    return b0


def head_params(L, rng, alpha_targets, beta_targets):
    """Parameters as tests/test_gpu_roach.py::make_case builds them, with zero head weights: the
    concentrations are those of the biases in every row, whatever the observation. Returns (params,
    alpha fp32 [A], beta fp32 [A]) with the concentrations the reference would form."""
    O_, A, H = L.O, L.A, L.H
    assert len(alpha_targets) == A and len(beta_targets) == A
    p = np.zeros(L.P, np.float32)
    for t in range(L.ntensors):
        o, n = L.t_off[t], L.t_len[t]
        p[o:o + n] = rng.standard_normal(n).astype(np.float32) * 0.1
    p[L.hi], p[L.lo] = HI, LO
    p[L.omean:L.omean + O_] = rng.standard_normal(O_) * 0.2
    p[L.ostd:L.ostd + O_] = rng.uniform(0.8, 1.5, O_)
    for tr in (L.critic, L.actor):
        p[tr[0]:tr[0] + H * O_] = rng.standard_normal(H * O_) / np.sqrt(O_)
        p[tr[4]:tr[4] + H * H] = rng.standard_normal(H * H) / np.sqrt(H)
        p[tr[2]:tr[2] + H] = rng.uniform(0.8, 1.2, H)
        p[tr[6]:tr[6] + H] = rng.uniform(0.8, 1.2, H)
    ba = np.array([bias_of(t) for t in alpha_targets], np.float32)
    bb = np.array([bias_of(t) for t in beta_targets], np.float32)
    for w, b, v in ((L.aW3, L.ab3, ba), (L.bW3, L.bb3, bb)):
        p[w:w + A * H] = 0.0
        p[b:b + A] = v
    return p.astype(np.float32), conc_of_bias(ba), conc_of_bias(bb)


# ------------------------------------------------------------------------------------------------
# scale_action and the deterministic actions, in fp32 as every copy computes them
# ------------------------------------------------------------------------------------------------
def scale_action(action, lo=LO, hi=HI):
    """scale_action (ac:251-260) in fp32: (a - lo) / (hi - lo) * (1 - 0) + 0, clamp(1e-7f, 1.0f + 1e-7f)."""
    a = np.asarray(action, np.float32)
    lo, hi, one, zero = np.float32(lo), np.float32(hi), np.float32(1), np.float32(0)
    s = ((a - lo) / (hi - lo) * (one - zero) + zero).astype(np.float32)
    return np.minimum(np.maximum(s, np.float32(1e-7)), one + np.float32(1e-7)).astype(np.float32)


def unscale_action(s, lo=LO, hi=HI):
    s = np.asarray(s, np.float32)
    lo, hi = np.float32(lo), np.float32(hi)
    return ((s - np.float32(0)) / (np.float32(1) - np.float32(0)) * (hi - lo) + lo).astype(np.float32)


def mean01(al, be):
    al, be = np.asarray(al, np.float32), np.asarray(be, np.float32)
    return (al / (al + be)).astype(np.float32)


def roach01(al, be):
    """Beta::roach_deterministic (rl_utils.h:112-131) in fp32."""
    al, be = np.asarray(al, np.float32), np.asarray(be, np.float32)
    one = np.float32(1)
    with np.errstate(invalid="ignore", divide="ignore"):
        mode = (al - one) / (al + be - np.float32(2))
    return np.where((al > 1) & (be > 1), mode,
                    np.where((al <= 1) & (be > 1), np.float32(0),
                             np.where((al > 1) & (be <= 1), one, al / (al + be)))).astype(np.float32)


# ------------------------------------------------------------------------------------------------
# the float64 restatement
# ------------------------------------------------------------------------------------------------
def beta_fp64(al, be, s):
    """Per (row, action) item in float64 torch, from the fp32 concentrations and the fp32 s exactly as the
    kernels hold them: log-prob (xlogy semantics), entropy, their derivatives in alpha and beta (xlogy's
    backward in its first argument is log y, also where that argument is 0), and for each the sum of the
    absolute values of its addends (mag_*). alpha + beta is the fp32 sum, as the reference and every copy
    form it before lgamma / digamma. d lp / d s is `dlp_ds`."""
    al = torch.from_numpy(np.array(al, np.float32)).double()
    be = torch.from_numpy(np.array(be, np.float32)).double()
    s = torch.from_numpy(np.array(s, np.float32)).double()
    al, be, s = torch.broadcast_tensors(al, be, s)
    # alpha + beta as every copy and the reference hold it: the fp32 sum (concentration_.sum(-1))
    ab = (al.float() + be.float()).double()
    one_s = 1.0 - s   # exact in fp64 for every fp32 s
    lga, lgb, lgab = torch.lgamma(al), torch.lgamma(be), torch.lgamma(ab)
    psa, psb, psab = torch.digamma(al), torch.digamma(be), torch.digamma(ab)
    ta, tb, tab = torch.polygamma(1, al), torch.polygamma(1, be), torch.polygamma(1, ab)
    xa, xb = torch.xlogy(al - 1, s), torch.xlogy(be - 1, one_s)
    out = {"alpha": al, "beta": be, "s": s}
    out["lp"] = xa + xb + lgab - lga - lgb
    out["mag_lp"] = xa.abs() + xb.abs() + lgab.abs() + lga.abs() + lgb.abs()
    e = [lga, lgb, -lgab, -(al - 1) * psa, -(be - 1) * psb, (ab - 2) * psab]
    out["ent"] = sum(e)
    out["mag_ent"] = sum(t.abs() for t in e)
    zero = torch.zeros_like(s)
    # xlogy's backward in its first argument: log(y), zero only where x == 0 and y <= 0
    ls = torch.where((al == 1) & (s <= 0), zero, torch.log(s))
    l1s = torch.where((be == 1) & (one_s <= 0), zero, torch.log(one_s))
    out["dlp_da"], out["mag_dlp_da"] = ls + psab - psa, ls.abs() + psab.abs() + psa.abs()
    out["dlp_db"], out["mag_dlp_db"] = l1s + psab - psb, l1s.abs() + psab.abs() + psb.abs()
    # the entropy's derivative as the reference's autograd adds it up: digamma(a) from lgamma(a) and again,
    # negated, from (a - 1) digamma(a), and the same pair at a + b; they cancel only up to their rounding
    out["dent_da"] = (ab - 2) * tab - (al - 1) * ta
    out["mag_dent_da"] = ((ab - 2) * tab).abs() + ((al - 1) * ta).abs() + 2 * psa.abs() + 2 * psab.abs()
    out["dent_db"] = (ab - 2) * tab - (be - 1) * tb
    out["mag_dent_db"] = ((ab - 2) * tab).abs() + ((be - 1) * tb).abs() + 2 * psb.abs() + 2 * psab.abs()
    out["dlp_ds"] = torch.where(al != 1, (al - 1) / s, zero) - torch.where(be != 1, (be - 1) / one_s, zero)
    out["mean"] = al / ab
    return out


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, np.float32))).astype(np.float64)


def row_bounds(ref, factor=2.0, stored_action=None, lo=LO, hi=HI, s_ulps=0.0):
    """The per-row bound of log-prob and entropy (module docstring) from beta_fp64's dict of [n, A] items.
    stored_action: the stored fp32 actions, for samples judged from the buffers. s_ulps: for the mean and
    the roach action, which a copy forms itself from its own concentrations, that many ulps of s through
    d lp / d s."""
    al32, be32 = ref["alpha"].numpy().astype(np.float32), ref["beta"].numpy().astype(np.float32)
    ua, ub = ulp32(al32), ulp32(be32)
    n = lambda k: ref[k].numpy()  # noqa: E731
    out = {}
    for q, da, db in (("lp", "dlp_da", "dlp_db"), ("ent", "dent_da", "dent_db")):
        b = FLOOR + factor * K_REF[q] * U * n("mag_" + q).sum(-1)
        b = b + factor * (np.abs(n(da)) * ua + np.abs(n(db)) * ub).sum(-1)
        out[q] = b
    if stored_action is not None:
        ds = ulp32(stored_action) / (hi - lo)
        out["lp"] = out["lp"] + (np.abs(n("dlp_ds")) * ds).sum(-1)
    if s_ulps:
        out["lp"] = out["lp"] + (np.abs(n("dlp_ds")) * s_ulps * ulp32(n("s").astype(np.float32))).sum(-1)
    return out


# ------------------------------------------------------------------------------------------------
# the reference's fp32 arithmetic (the same formulas in torch float32, gradients by autograd)
# ------------------------------------------------------------------------------------------------
def beta_torch_fp32(al, be, s):
    """log-prob, entropy and their (alpha, beta) gradients per item as torch float32 on the CPU computes
    them: torch.distributions.Beta's formulas (Dirichlet log_prob / entropy) with autograd."""
    al = torch.tensor(np.asarray(al, np.float32), requires_grad=True)
    be = torch.tensor(np.asarray(be, np.float32), requires_grad=True)
    s = torch.as_tensor(np.asarray(s, np.float32))
    ab = al + be
    lp = torch.xlogy(al - 1, s) + torch.xlogy(be - 1, 1 - s) + torch.lgamma(ab) - torch.lgamma(al) - torch.lgamma(be)
    ent = (torch.lgamma(al) + torch.lgamma(be) - torch.lgamma(ab) - (al - 1) * torch.digamma(al)
           - (be - 1) * torch.digamma(be) + (ab - 2) * torch.digamma(ab))
    dla, dlb = torch.autograd.grad(lp.sum(), (al, be), retain_graph=True)
    dea, deb = torch.autograd.grad(ent.sum(), (al, be))
    return {"lp": lp.detach(), "ent": ent.detach(), "dlp_da": dla, "dlp_db": dlb, "dent_da": dea, "dent_db": deb}


# ------------------------------------------------------------------------------------------------
# given-action cases of the forward checks
# ------------------------------------------------------------------------------------------------
GIVEN = ("lo", "s1e-7", "s1e-3", "mode", "mean", "s1-1e-3", "smax", "below_lo", "above_hi", "hi")


def given_actions(al, be, n, lo=LO, hi=HI):
    """[n, A] fp32 actions and the case name of each row: row r takes case (r + n) % 10 of GIVEN, so one
    row, three rows and seventy rows start at different cases and seventy rows hold each case seven times."""
    al, be = np.asarray(al, np.float32), np.asarray(be, np.float32)
    A = al.size
    with np.errstate(invalid="ignore", divide="ignore"):
        mode = np.where((al > 1) & (be > 1), (al - 1.0) / (al + be - 2.0), al / (al + be)).astype(np.float32)
    table = {
        "lo": np.full(A, lo, np.float32), "hi": np.full(A, hi, np.float32),
        "s1e-7": unscale_action(np.full(A, 1e-7, np.float32), lo, hi),
        "s1e-3": unscale_action(np.full(A, 1e-3, np.float32), lo, hi),
        "mode": unscale_action(mode, lo, hi), "mean": unscale_action(mean01(al, be), lo, hi),
        "s1-1e-3": unscale_action(np.full(A, 1 - 1e-3, np.float32), lo, hi),
        "smax": unscale_action(np.full(A, S_MAX, np.float32), lo, hi),
        "below_lo": np.full(A, lo - 0.25 * (hi - lo), np.float32),
        "above_hi": np.full(A, hi + 0.25 * (hi - lo), np.float32),
    }
    names = [GIVEN[(r + n) % len(GIVEN)] for r in range(n)]
    return np.stack([table[k] for k in names]).astype(np.float32), names


# ------------------------------------------------------------------------------------------------
# sampler: closed-form moments (exact rationals of the fp32 concentrations) and the 5-sigma rule
# ------------------------------------------------------------------------------------------------
def beta_central_moments(al32, be32, kmax=6):
    """Central moments m_0..m_kmax of Beta(alpha, beta) as floats, computed exactly in rationals (the raw
    moments cancel to 1e-18 of themselves at (1000, 1), beyond fp64)."""
    a, b = Fraction(float(np.float32(al32))), Fraction(float(np.float32(be32)))
    raw = [Fraction(1)]
    for k in range(kmax):
        raw.append(raw[-1] * (a + k) / (a + b + k))
    mu = raw[1]
    from math import comb
    cen = [sum(comb(k, j) * raw[j] * (-mu) ** (k - j) for j in range(k + 1)) for k in range(kmax + 1)]
    return float(mu), [float(c) for c in cen]


def moment_check(s, al32, be32, sigmas=5.0):
    """The first three sample moments of s (fp32 samples of one action dimension) against the closed forms:
    |mean - mu| < 5 sigma / sqrt(n), and the variance and the third central moment by the same rule with
    their own sampling variances (leading order in 1 / n): Var(m2^) = (m4 - m2^2) / n and
    Var(m3^) = (m6 - m3^2 - 6 m4 m2 + 9 m2^3) / n. Returns the three ratios |deviation| / (5 sd)."""
    x = np.asarray(s, np.float64)
    n = x.size
    mu, m = beta_central_moments(al32, be32)
    d = x - x.mean()
    dev = [abs(x.mean() - mu), abs((d ** 2).mean() - m[2] * (n - 1) / n), abs((d ** 3).mean() - m[3])]
    var = [m[2] / n, (m[4] - m[2] ** 2) / n, (m[6] - m[3] ** 2 - 6 * m[4] * m[2] + 9 * m[2] ** 3) / n]
    return [dv / (sigmas * np.sqrt(v)) for dv, v in zip(dev, var)]


def oracle_samples(al32, be32, a, E, T, seed=1, rank=0, env_base=0, step0=0):
    """The oracle's Beta sampler at the Philox counters the kernels use for action dimension a of env e at
    step t: [T, E] fp32."""
    import ctypes as C
    f = Orc.lib().orc_beta_sample01
    f.restype = C.c_float
    f.argtypes = [C.c_float, C.c_float, C.c_uint64, C.c_int, C.c_long, C.c_long, C.c_int]
    return np.array([[f(float(al32), float(be32), seed, rank, env_base + e, step0 + t, a) for e in range(E)]
                     for t in range(T)], np.float32)


# ------------------------------------------------------------------------------------------------
# the update's loss over a minibatch, restated in fp64 for the head-bias gradients
# ------------------------------------------------------------------------------------------------
def softplus_d64(b32):
    b = np.asarray(b32, np.float32).astype(np.float64)
    return np.where(b > 20.0, 1.0, 1.0 / (1.0 + np.exp(-b)))


def update_fp64(ref, old_logp, adv, clip, ent_coef, ba32, bb32, extra_lp_bound=0.0, factor=2.0):
    """One minibatch of M rows with advantage normalisation off: the clipped surrogate and the entropy bonus
    (ac:816-875) on beta_fp64's [M, A] items, and the head-bias gradients. With zero head weights element a of
    a head-bias gradient is exactly sum_rows d loss / d pre[row, a] = sum_rows (g_logp dlp + g_ent dent)
    softplus'(bias[a]).

    Bounds (factor f = 2, a kernel; 1, the oracle). Gradient element: f K_REF 2^-24 sum_rows sum |addends|
    (each addend weighted by |g_logp| or |g_ent| and softplus') plus the first-order effect of each row's log-prob bound on its ratio,
    |g_logp| (e^bound - 1) |dlp|, plus M FLT_MIN (nothing below the smallest normal fp32 is resolved: the
    bias -100 has softplus' = 4e-44). Statistics: the mean over rows of each row's bound, through the same
    first-order effect where the ratio enters, plus 1e-6 of the mean magnitude for the fp32 row sums.
    extra_lp_bound: added to each row's log-prob bound (the action round trip of stored samples)."""
    M = old_logp.shape[0]
    n = lambda k: ref[k].numpy()  # noqa: E731
    rb = row_bounds(ref, factor)
    lpb = rb["lp"] + extra_lp_bound
    lp, ent = n("lp").sum(-1), n("ent").sum(-1)
    logratio = lp - old_logp.astype(np.float64)
    ratio = np.exp(logratio)
    an = adv.astype(np.float64)
    inr = (ratio >= 1 - clip) & (ratio <= 1 + clip)
    pg1, pg2 = -an * ratio, -an * np.clip(ratio, 1 - clip, 1 + clip)
    w1 = np.where(pg1 > pg2, 1.0, np.where(pg1 == pg2, 0.5, 0.0))
    g_logp = (w1 * (-an) + (1 - w1) * (-an) * inr) * ratio / M
    g_ent = -ent_coef / M
    dg_logp = np.abs(g_logp) * np.expm1(lpb)
    out = {"ratio": ratio, "lp_bound": lpb, "logratio": logratio}
    # distance of each row's log-ratio from the clip edges, in units of its log-prob bound (> 1: the row
    # is on the same side of both edges in fp64 and in any copy within its bound)
    edges = np.log(np.array([1 - clip, 1 + clip]))
    out["edge_margin"] = np.abs(logratio[:, None] - edges[None, :]).min(1) / lpb
    for h, dl, de, sp in (("a", "dlp_da", "dent_da", softplus_d64(ba32)), ("b", "dlp_db", "dent_db", softplus_d64(bb32))):
        dlx, dex = n(dl), n(de)
        row = (g_logp[:, None] * dlx + g_ent * dex) * sp        # d loss / d pre[row, a]
        mag = np.abs(g_logp)[:, None] * n("mag_" + dl) * K_REF["dlp"] + abs(g_ent) * n("mag_" + de) * K_REF["dent"]
        row_bound = (factor * U * mag + dg_logp[:, None] * np.abs(dlx)) * sp
        out["row_g" + h], out["row_g" + h + "_bound"] = row, row_bound
        out["g" + h] = row.sum(0)
        out["g" + h + "_bound"] = row_bound.sum(0) + M * FLT_MIN
    pg = np.maximum(pg1, pg2)
    kl = (ratio - 1) - logratio
    out["stats"] = {"pg_loss": pg.mean(), "entropy": ent.mean(), "old_approx_kl": (-logratio).mean(),
                    "approx_kl": kl.mean(), "clipfrac": (np.abs(ratio - 1) > clip).mean()}
    # f(x) = e^x - 1 - x: f(x + d) - f(x) = e^x (e^d - 1 - d) + (e^x - 1) d
    dkl = ratio * (np.expm1(lpb) - lpb) + np.abs(ratio - 1) * lpb
    out["stats_bound"] = {"pg_loss": (np.abs(an) * ratio * np.expm1(lpb)).mean() + 1e-6 * np.abs(pg).mean(),
                          "entropy": rb["ent"].mean() + 1e-6 * np.abs(ent).mean(),
                          "old_approx_kl": lpb.mean() + 1e-6 * np.abs(logratio).mean(),
                          "approx_kl": dkl.mean() + 1e-6 * np.abs(kl).mean(), "clipfrac": 0.0}
    return out


def head_weight_grad(u, h, h2):
    """d loss / d W3 [A, H] of head h ("a" | "b") from update_fp64's per-row gradients and the actor's last
    hidden layer h2 [M, H] in fp64, with its element-wise bound: each row's bound times |h2|, plus each
    row's |gradient| times 2^-17 (|h2| + 1) for the trunk and the fp32 row sums. h2 is a LayerNorm output of
    unit scale behind a 256-term dot product whose |products| sum to about 8, in fp32 or split-bf16 pieces
    (2^-23 of each product dropped), divided by a standard deviation of about a half: its error is absolute
    at that scale, not relative to a unit that the ReLU leaves barely positive in a few rows."""
    g = np.einsum("ra,ri->ai", u["row_g" + h], h2)
    b = np.einsum("ra,ri->ai", u["row_g" + h + "_bound"], np.abs(h2))
    b = b + 2.0 ** -17 * np.einsum("ra,ri->ai", np.abs(u["row_g" + h]), np.abs(h2) + 1.0) + h2.shape[0] * FLT_MIN
    return g, b


def actor_h2_fp64(L, p, x):
    """The actor trunk of the LayerNorm-Beta agent in fp64 (fixed normalisation, Linear-LayerNorm-ReLU
    twice; tests/test_gpu_roach.py::actor_fp64 without the heads): the heads' input [n, H]."""
    import torch.nn.functional as F
    P = torch.from_numpy(p.astype(np.float64))
    H, O_ = L.H, L.O
    t = list(L.actor)
    h = (torch.from_numpy(x.astype(np.float64)) - P[L.omean:L.omean + O_]) / P[L.ostd:L.ostd + O_]
    for w, b, g, be, fan in ((t[0], t[1], t[2], t[3], O_), (t[4], t[5], t[6], t[7], H)):
        h = F.linear(h, P[w:w + H * fan].reshape(H, fan), P[b:b + H])
        h = F.relu(F.layer_norm(h, (H,), P[g:g + H], P[be:be + H], 1e-5))
    return h.numpy()


def update_rows(al, be, M, rng, lo=LO, hi=HI):
    """[M, A] fp32 actions of the update cases: the given-action cases without the two whose log-prob the
    reference itself makes -inf / NaN (action = hi, action above hi), then uniform actions."""
    cases = [c for c in GIVEN if c not in ("hi", "above_hi")]
    acts, names = given_actions(al, be, len(GIVEN), lo, hi)
    rows = [acts[names.index(c)] for c in cases]
    k = 7 * len(cases)
    a = np.empty((M, len(al)), np.float32)
    for r in range(M):
        a[r] = rows[r % len(cases)] if r < k else rng.uniform(lo + 1e-3, hi - 1e-3, len(al))
    return a


OLD_LOGP_OFFSETS = (0.0, 0.05, -0.05, 0.5, -0.5)


def update_case(al, be, M, rng, lo=LO, hi=HI):
    """(actions [M, A], beta_fp64 items, old_logp fp32 [M], advantages fp32 [M] of both signs): old_logp is
    fp32(fp64 log-prob) plus an offset from {0, +-0.05, +-0.5}, which keeps every row's ratio away from the
    clip edges 1 +- 0.2 (log 0.8 = -0.223, log 1.2 = 0.182) by more than its log-prob bound."""
    act = update_rows(al, be, M, rng, lo, hi)
    ref = beta_fp64(np.broadcast_to(al, act.shape), np.broadcast_to(be, act.shape), scale_action(act, lo, hi))
    lp = ref["lp"].numpy().sum(-1)
    off = np.array([OLD_LOGP_OFFSETS[r % len(OLD_LOGP_OFFSETS)] for r in range(M)])
    old = (lp.astype(np.float32) + off.astype(np.float32)).astype(np.float32)
    adv = rng.standard_normal(M).astype(np.float32)
    adv[::2] = np.abs(adv[::2]); adv[1::2] = -np.abs(adv[1::2])
    return act, ref, old, adv
