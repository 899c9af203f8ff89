"""The committed cases of the 4-DoF essential-graph tests, the model runs they share (computed once per process, never modified) and the
bounds the device is held to.  TEST INFRASTRUCTURE ONLY.

Sizes are the smallest at which each path of the kernels can go wrong: 2 vertices with one edge (one of them fixed), a 3-vertex chain, 7,
8 and 9 active edges on 4 vertices (one below, at and one above the 8 edges a workgroup of the linearise kernel takes; pairs repeat, so
several edges lie between one pair), a 10-keyframe loop (n = 40: two 32-column panels) with an edge between two fixed vertices, 120 and
121 free keyframes (480 / 484 unknowns: the last single-workgroup size and the first many-workgroup one), and a damped run with more
than six accepted iterations.

The residual is close to linear in yaw and translation, and with lambda = 1e-50 max|H(j,j)| the first trial of an iteration is a
Gauss-Newton step: the extended-precision model gains all but 1e-9 of chi2 within two or three iterations, and every later decision
is rounding noise.  MIN_PREFIX is therefore 2 for the undamped cases; the damped cases (lambda_init = 30 or more on a graph whose
max|H(j,j)| is some thousand) converge linearly and have a prefix of six and more iterations, all accepted.

Conditions on every case (test_essential_graph4dof_model.py asserts them; a case that misses one gets another seed or drift, never
another condition): the extended-precision run has a decisive prefix of at least the case's minimum, the float64 model decides like it
over that prefix, and no evaluated branch argument (d of ExpSO3, |sin theta| of LogSO3, both against 1e-5) lies within MIN_MARGIN."""
import functools
import numpy as np
import essential_graph4dof_model as em
import synth_essential_graph4dof as sg
from ba_step_model import K as K_RULE, within_bound  # noqa: F401

LD = np.longdouble
MIN_PREFIX = 2
MIN_PREFIX_DAMPED = 6
MIN_MARGIN = 1e-7

# name -> (generator, generator arguments, lambda_init (0: computed), iterations)
CASES = {
    "c2": ("chain", dict(seed=1, n_vertices=2), 0.0, 20),
    "c3": ("chain", dict(seed=2, n_vertices=3), 0.0, 20),
    "e7": ("chain", dict(seed=3, n_vertices=4, n_edges=7), 0.0, 20),
    "e8": ("chain", dict(seed=3, n_vertices=4, n_edges=8), 0.0, 20),
    "e9": ("chain", dict(seed=3, n_vertices=4, n_edges=9), 0.0, 20),
    "v10": ("loop", dict(seed=1, n_free=10), 0.0, 20),
    "v10_damped": ("loop", dict(seed=1, n_free=10), 300.0, 12),
    "v40": ("loop", dict(seed=2, n_free=40), 0.0, 20),
    "v120": ("loop", dict(seed=1, n_free=120, yaw_drift=3e-4, trans_drift=3e-3), 0.0, 6),
    "v121": ("loop", dict(seed=2, n_free=121, yaw_drift=3e-4, trans_drift=3e-3), 0.0, 6),
}
DAMPED = ("v10_damped",)
RAGGED = ("v10", "c2", "e9")
GROUPS = ("R", "t", "chi", "lam")


@functools.lru_cache(maxsize=None)
def make(name):
    kind, kw, lam, its = CASES[name]
    g = sg.chain(**kw) if kind == "chain" else sg.make_graph(**kw)
    return g, em.default_params(its, lambda_init=lam)


def min_prefix(name):
    return MIN_PREFIX_DAMPED if name in DAMPED else MIN_PREFIX


@functools.lru_cache(maxsize=None)
def model_runs(name, iterations=None):
    """(float64 run, extended-precision run, decisive prefix)."""
    g, prm = make(name)
    prm = dict(prm)
    if iterations is not None:
        prm["iterations"] = iterations
    r64 = em.optimize(g, g["state"], prm, np.float64)
    rld = em.optimize(g, g["state"], prm, LD)
    return r64, rld, em.decisive_prefix(rld["trace"])


def group_values(est, chi, lam, free):
    e = np.asarray(est, LD).reshape(-1, 36)[np.asarray(free, bool)]
    return dict(R=np.concatenate([e[:, 0:9], e[:, 12:21]], 1).reshape(-1), t=np.concatenate([e[:, 9:12], e[:, 21:24]], 1).reshape(-1),
                chi=np.array([chi], LD), lam=np.array([lam], LD))


def run_groups(run):
    return group_values(run["est"], run["chi_last"], run["lam"], run["free"])


def group_errors(a, ref):
    return {g: (float(np.max(np.abs(np.asarray(a[g], LD) - np.asarray(ref[g], LD)))) if len(ref[g]) else 0.0) for g in GROUPS}


def k_rule(dev, r64, rld, groups=GROUPS, storage_floor=2.0 ** -52):
    """-> (ok, {group: (device error, bound, float64-model error, ratio)}).  The project's K rule (ba_step_model.within_bound, K = 128):
    e_device <= K (e_float64_model + floor), both errors against the extended-precision model, floor = 2^-52 max|value| (what storing
    the result in float64 costs)."""
    ref = run_groups(rld)
    e64, edev = group_errors(run_groups(r64), ref), group_errors(dev, ref)
    rep, ok = {}, True
    for g in groups:
        floor = storage_floor * float(np.max(np.abs(ref[g])))
        rep[g] = (edev[g], K_RULE * (e64[g] + floor), e64[g], edev[g] / (e64[g] + floor))
        ok = ok and within_bound(edev[g], e64[g], floor, K_RULE)
    return ok, rep


def past_prefix_slack(name):
    """What a whole run's final chi2 may exceed the chi2 at the end of the decisive prefix by (essential_graph_cases.past_prefix_slack's
    rule): past the prefix a trial moves chi2 by less than 1e-9 of it and is accepted or rejected by rounding; chi2 cannot rise, so the
    distance is what the float64 model itself shows against the extended one, under the K rule with the float64 floor.  Computed from
    the two model runs, never from the device."""
    r64, rld, pre = model_runs(name)
    ref = float(rld["trace"][pre - 1]["chi"] - rld["trace"][pre - 1]["dchi"])
    k64 = min(pre, len(r64["trace"])) - 1
    shown = max(abs(float(r64["trace"][k64]["chi"] - r64["trace"][k64]["dchi"]) - ref), abs(float(r64["chi_last"]) - ref), abs(float(rld["chi_last"]) - ref))
    return ref, K_RULE * (shown + 2.0 ** -52 * abs(ref))
