"""The committed cases of the essential-graph tests, the model runs they share (computed once per process, never modified) and the
bounds the device is held to.  TEST INFRASTRUCTURE ONLY.

Sizes are the smallest at which each path of the kernels can go wrong: 2, 5, 10 free vertices (n = 14, 35, 70: one to three 32-column
panels), 68 and 69 (476 / 483: the last single-workgroup size and the first many-workgroup one), 75 (525: a ragged last panel and a
ragged 64-tile), 150 (1050; held to the float64 model only).  The reference runs optimize(20); the larger fixed-scale cases run 6
iterations, the larger free-scale one 3 (its whole run is the decisive prefix: every further iteration adds some thirty evaluations of
every edge, and with them chances for one of some hundred residuals to come within 1e-6 of a threshold).

Conditions on every case (test_essential_graph_model.py asserts them; a case that misses one gets another seed or drift, never another
condition): the extended-precision run has a decisive prefix of at least MIN_PREFIX iterations, the float64 model decides like it over
that prefix, and no evaluated branch argument of Sim3::log or the exponential lies within MIN_MARGIN of its threshold.
Which drifts meet them: with the start value lambda = 1e-16 the first trial of an iteration is a Gauss-Newton step; on a loop with
several per cent of scale drift it overshoots, lambda is doubled, quadrupled, ... up to a dozen times, and the trial that is finally
taken has rho barely above zero -- such decisions flip with the last bits and the float64 model leaves the extended one.  And with some
hundred edges a drift of a milliradian per keyframe puts some edge's residual rotation into the band 4.2 .. 4.7 mrad (d within 1e-6 of
1 - 1e-5) at one of the ~30 x trials evaluations.  The larger cases therefore drift little (rotations stay in the small-angle branch of
the logarithm throughout, scale residuals stay a decade above 1e-5); the small cases carry the large drifts and both sides of both
thresholds.  Free scale at 68, 69 and 75 vertices: of some hundred (seed, drift) pairs tried per size, with three iterations, seeds 2,
30 and 31 meet the conditions (3 per cent of scale drift and 12 mrad of rotation drift per keyframe: every first trial is accepted); on
them the float64 model itself is 1e-4 .. 3e-3 relative off the extended one in chi2, which the K rule and the slack records carry.  At
150 vertices none of 234 pairs did, and with 3 per cent of scale drift per keyframe the scales of such a graph span a factor of
ninety: one iteration of the float64 model is already 0.5 m off the extended one.  A smaller scale drift (0.3 and 0.6 per cent per
keyframe, three rotation drifts, 40 seeds each: 240 more pairs) does not help: the first trials overshoot again (13 to 23 trials in
three iterations), and some residual lands within 1e-7 of a threshold on every one.  That size has its fixed-scale case only."""
import functools
import numpy as np
import essential_graph_model as em
import synth_essential_graph as sg
from ba_step_model import K as K_RULE, within_bound

LD = np.longdouble
MIN_PREFIX = 3
MIN_MARGIN = 1e-6

# name -> (free vertices, fix_scale, iterations, generator arguments)
CASES = {
    "v2": (2, False, 20, dict(seed=2, rot_drift=0.003, scale_drift=0.012)),
    "v5": (5, False, 20, dict(seed=2, rot_drift=0.003, scale_drift=0.03)),
    "v5_fix": (5, True, 20, dict(seed=3, rot_drift=0.012)),
    "v10": (10, False, 20, dict(seed=2, rot_drift=0.03, scale_drift=0.012)),
    "v10_fix": (10, True, 20, dict(seed=1, rot_drift=0.03)),
    "v68": (68, False, 3, dict(seed=2, rot_drift=1.2e-2, scale_drift=0.03, trans_drift=1e-2)),
    "v68_fix": (68, True, 6, dict(seed=1, rot_drift=2e-4, trans_drift=1e-2)),
    "v69": (69, False, 3, dict(seed=30, rot_drift=1.2e-2, scale_drift=0.03, trans_drift=1e-2)),
    "v69_fix": (69, True, 6, dict(seed=3, rot_drift=1e-4, trans_drift=3e-2)),
    "v75": (75, False, 3, dict(seed=31, rot_drift=1.2e-2, scale_drift=0.03, trans_drift=1e-2)),
    "v75_fix": (75, True, 6, dict(seed=1, rot_drift=3e-4, trans_drift=1e-2)),
    "v150_fix": (150, True, 6, dict(seed=6, rot_drift=2e-4, trans_drift=3e-2)),
}
LARGE = ("v150_fix",)                                        # held to the float64 model only
RAGGED = ("v5", "v10_fix", "v2")
GROUPS = ("q", "t", "s", "chi", "lam")


@functools.lru_cache(maxsize=None)
def make(name):
    n_free, fix_scale, its, kw = CASES[name]
    return sg.make_graph(n_free=n_free, fix_scale=fix_scale, **kw), em.default_params(its, fix_scale)


@functools.lru_cache(maxsize=None)
def model_runs(name, iterations=None):
    """(float64 run, extended-precision run or None for a LARGE case, decisive prefix or None)."""
    g, prm = make(name)
    prm = dict(prm)
    if iterations is not None:
        prm["iterations"] = iterations
    r64 = em.optimize(g, g["sim3"], prm, np.float64)
    if name in LARGE:
        return r64, None, None
    rld = em.optimize(g, g["sim3"], prm, LD)
    return r64, rld, em.decisive_prefix(rld["trace"])


def _canon(est):
    """q and -q are one rotation: w >= 0."""
    est = np.array(est, LD).reshape(-1, 8)
    est[:, :4] *= np.where(est[:, 3:4] < 0, -1, 1)
    return est


def group_values(est, chi, lam, free):
    e = _canon(est)[np.asarray(free, bool)]
    return dict(q=e[:, :4].reshape(-1), t=e[:, 4:7].reshape(-1), s=e[:, 7], chi=np.array([chi], LD), lam=np.array([lam], LD))


def run_groups(run):
    return group_values(run["est"], run["chi_last"], run["lam"], run["free"])


def group_errors(a, ref):
    return {g: (float(np.max(np.abs(np.asarray(a[g], LD) - np.asarray(ref[g], LD)))) if len(ref[g]) else 0.0) for g in GROUPS}


def k_rule(dev, r64, rld, groups=GROUPS):
    """-> (ok, {group: (device error, bound, float64-model error, ratio)}).  The project's K rule (ba_step_model.within_bound, K = 128):
    e_device <= K (e_float64_model + floor), both errors against the extended-precision model, floor = 2^-52 max|value| (what storing
    the result in float64 costs)."""
    ref = run_groups(rld)
    e64, edev = group_errors(run_groups(r64), ref), group_errors(dev, ref)
    rep, ok = {}, True
    for g in groups:
        floor = 2.0 ** -52 * float(np.max(np.abs(ref[g])))
        rep[g] = (edev[g], K_RULE * (e64[g] + floor), e64[g], edev[g] / (e64[g] + floor))
        ok = ok and within_bound(edev[g], e64[g], floor, K_RULE)
    return ok, rep


# (chi2 at the end of the decisive prefix, slack) per case as past_prefix_slack() measured them when the case was committed;
# test_essential_graph_model.py holds the function to these records (a drift of the model shows there), the GPU test uses the records
PAST_PREFIX_SLACK = {
    "v2": (0.024811005495841653, 1.29e-11),
    "v5": (1.2376956137957551, 0.000152),
    "v5_fix": (0.081494985268619563, 1.58e-10),
    "v10": (3.4461936240021971, 4.8e-06),
    "v10_fix": (0.96756488130032869, 8.3e-09),
    "v68": (20.421367491615879, 0.627),
    "v68_fix": (0.001707943645530638, 4.75e-12),
    "v69": (58.818215221522671, 1.8),
    "v75": (29.995991247324813, 11.1),
    "v69_fix": (0.0018117850181421039, 2.05e-12),
    "v75_fix": (0.0035879704515970833, 2.12e-11),
}


def past_prefix_slack(name):
    """What a whole run's final chi2 may exceed the chi2 at the end of the decisive prefix by.  Past the prefix a trial moves chi2 by
    less than 1e-9 of it and is accepted or rejected by rounding; chi2 cannot rise (a trial that raises it is rejected), so the
    distance is what the float64 model itself shows against the extended one -- its chi2 at the end of the prefix and at the end of
    the run against the extended model's chi2 at the end of the prefix -- under the K rule with the float64 floor."""
    r64, rld, pre = model_runs(name)
    ref = float(rld["trace"][pre - 1]["chi"] - rld["trace"][pre - 1]["dchi"])
    shown = max(abs(float(r64["trace"][min(pre, len(r64["trace"])) - 1]["chi"] - r64["trace"][min(pre, len(r64["trace"])) - 1]["dchi"]) - ref),
                abs(float(r64["chi_last"]) - ref), abs(float(rld["chi_last"]) - ref))
    return ref, K_RULE * (shown + 2.0 ** -52 * abs(ref))


@functools.lru_cache(maxsize=None)
def largest_model_distance(fix_scale):
    """The largest distance between the float64 and the extended-precision model's final state over the cases of ONE scale setting
    that have both runs (q, t, s: absolute; chi_rel: |chi2_64 - chi2_ld| / chi2_ld); K times it bounds a LARGE case's distance to the
    float64 model.  Per setting, because the free-scale cases are conditioned a thousand times worse than the fixed-scale ones
    (t: 3.4e-3 m against 3.8e-7 m): their distance says nothing about a fixed-scale graph."""
    out = {g: 0.0 for g in ("q", "t", "s", "chi_rel")}
    for name in CASES:
        if name in LARGE or CASES[name][1] != bool(fix_scale):
            continue
        r64, rld, _ = model_runs(name)
        e = group_errors(run_groups(r64), run_groups(rld))
        for g in ("q", "t", "s"):
            out[g] = max(out[g], e[g])
        out["chi_rel"] = max(out["chi_rel"], e["chi"] / abs(float(rld["chi_last"])))
    return out
