"""The named cases of the InertialOptimization tests, the model runs they share (computed once per process) and the project's K rule
(tests/ba_step_model.py: the device may be K = 128 times as far from the extended-precision model as the float64 model is).
TEST INFRASTRUCTURE ONLY."""
import functools
import numpy as np
import inertial_opt_model as iom
import synth_inertial_opt as sio
from ba_step_model import K

LD = np.longdouble
# family -> the arguments of default_params / orbhip.inertial_opt_params: (overload, mono, fixed_vel, priorG, priorA)
FAMILIES = {
    "a_mono": (0, True, False, 0.0, 0.0),            # priorG = 0: lambda_0 from g2o's rule
    "a_mono_prior": (0, True, False, 1e2, 1e6),
    "a_stereo": (0, False, False, 1e2, 1e6),
    "a_fixed": (0, True, True, 1e2, 1e6),
    "b": (1, False, False, 1.0, 1e2),
    "d": (3, False, False, 0.0, 0.0),
}
OVERLOAD_OF = {f: ("a" if f.startswith("a") else f) for f in FAMILIES}
# the generator's cases for the full runs: (family, keyframes, seed); their decisive prefix is at least 5 iterations (asserted)
FULL_CASES = [("a_mono", 10, 1), ("a_mono_prior", 65, 1), ("a_mono_prior", 10, 2), ("a_stereo", 10, 2), ("a_fixed", 10, 1), ("b", 10, 12)]
GROUPS = ("Rwg", "scale", "bg", "ba", "vel", "chi", "lam")


def make(family, n, seed, gaps=()):
    """The map of a case (synth_inertial_opt layout)."""
    r = np.random.default_rng(1000 + seed)
    small = (r.normal(0, 0.003, 3), r.normal(0, 0.004, 3))
    large = (r.normal(0, 0.1, 3), r.normal(0, 0.02, 3))
    if family == "a_mono":
        return sio.make_map(seed, n, mono=True, noise=1.0, gaps=gaps)
    if family == "a_mono_prior":
        return sio.make_map(seed, n, mono=True, noise=1.0, bias_true=small, gaps=gaps)
    if family == "a_stereo":
        return sio.make_map(seed, n, mono=False, noise=1.0, bias_true=large, gaps=gaps)
    if family == "a_fixed":                                 # fixed biases that are not zero: the prior edges must stay out of chi2
        mp = sio.make_map(seed, n, mono=True, noise=1.0, bias_true=small, gaps=gaps)
        mp["glob"][10:13] = small[0] + r.normal(0, 0.001, 3); mp["glob"][13:16] = small[1] + r.normal(0, 0.002, 3)
        mp["kf"][:, 15:21] = mp["glob"][10:16]
        return mp
    if family == "b":
        return sio.make_map(seed, n, mono=False, noise=1.0, aligned=True, bias_true=large, gaps=gaps)
    if family == "d":
        return sio.refine_start(sio.make_map(seed, n, mono=True, scale_true=1.0, noise=1.0, gaps=gaps), 15.0, 1.4)
    raise KeyError(family)


def params(family, iterations=None):
    p = iom.default_params(*FAMILIES[family])
    if iterations is not None:
        p["iterations"] = iterations
    return p


@functools.lru_cache(maxsize=None)
def model_runs(family, n, seed, iterations=None, gaps=()):
    """(map, float64 run, extended-precision run) of a case; shared by the tests and never modified."""
    mp = make(family, n, seed, gaps)
    p = params(family, iterations)
    return mp, iom.optimize(mp, p, np.float64), iom.optimize(mp, p, LD)


def group_values(kf, glob, chi, lam):
    kf, glob = np.asarray(kf), np.asarray(glob)
    return dict(Rwg=glob[0:9], scale=glob[9:10], bg=glob[10:13], ba=glob[13:16], vel=kf[:, 12:15].reshape(-1), chi=np.array([chi]),
                lam=np.array([lam]))


def group_errors(a, ref):
    """max |a - ref| per group, in extended precision."""
    return {g: (float(np.max(np.abs(np.asarray(a[g]).astype(LD) - np.asarray(ref[g]).astype(LD)))) if len(np.atleast_1d(a[g])) else 0.0)
            for g in GROUPS}


def run_groups(r):
    return group_values(r["kf"], r["glob"], r["chi_last"], r["lam"])


PAST_PREFIX_ITERATIONS = 3


def past_prefix_slack(r64, rld, pre):
    """What the iterations past the decisive prefix may add to the end state.  There every accept / reject decision is rounding
    noise where a trial moves chi2 by less than 1e-9 of it (a trial that moves it by more is decided alike by everyone), so a run
    may take or leave those trial steps; an iteration past the prefix gains less than 1e-9 of chi2, far below the 1e-3 of LM's stop
    test, so at most PAST_PREFIX_ITERATIONS = 3 of them run before the three-bad-iterations stop.
    -> per group: 3 x the largest change such a trial proposed in either model run; chi2: 3 x 1e-9 chi2; lambda is decided by those
    trials alone and is not compared (None)."""
    out = {g: 0.0 for g in GROUPS}
    for r in (r64, rld):
        for it in r["trace"][pre:]:
            for g, v in it["step"].items():
                out[g] = max(out[g], PAST_PREFIX_ITERATIONS * float(v))
    out["chi"] = PAST_PREFIX_ITERATIONS * 1e-9 * abs(float(rld["trace"][pre - 1]["chi"] if pre else rld["chi_first"]))
    out["lam"] = None
    return out


def k_rule(dev, r64, rld, floors, slack=None):
    """-> (ok, {group: (device error, bound, float64 error)}): device error <= K * (e + storage floor), e = the float64 model's error or,
    where that is zero, the largest float64-model error of the overload; the storage floor is 2^-52 max|value|, what storing a result in
    float64 costs (the floor of tests/ba_step_model.py's within_bound: a float64 model that lands within a fraction of an ulp of the
    extended-precision value by luck measures no arithmetic).  slack: past_prefix_slack() for runs that go on past the decisive prefix."""
    ref = run_groups(rld)
    e64 = group_errors(run_groups(r64), ref)
    edev = group_errors(dev, ref)
    rep, ok = {}, True
    for g in GROUPS:
        base = e64[g] if e64[g] > 0 else floors[g]
        if len(np.atleast_1d(ref[g])):
            base += 2.0 ** -52 * float(np.max(np.abs(np.asarray(ref[g]).astype(LD))))
        bound = K * base
        if slack is not None:
            if slack[g] is None:
                continue
            bound += slack[g]
        rep[g] = (edev[g], bound, e64[g])
        ok = ok and edev[g] <= bound
    return ok, rep


def floors_of(cases):
    """Per overload and group: the largest float64-model error over the given cases [(family, n, seed, iterations, gaps)]."""
    out = {}
    for c in cases:
        _, r64, rld = model_runs(*c)
        e = group_errors(run_groups(r64), run_groups(rld))
        f = out.setdefault(OVERLOAD_OF[c[0]], {g: 0.0 for g in GROUPS})
        for g in GROUPS:
            f[g] = max(f[g], e[g])
    return out
