"""Rotation-histogram cases for every matcher that owns one (ORBmatcher.cc: the rot / bin lines of each search and ComputeThreeMaxima,
:2307-2348).  TEST INFRASTRUCTURE ONLY, shared by test_rotation_cases.py (oracle alone: each case is the case it claims to be) and
test_gpu_rotation.py (device against oracle).

A case is what the matcher's existing builder makes, with the angle columns overwritten: the first (query) side gets angle 0, a keypoint
of the second side (360 - 30 b) mod 360 with b drawn from the profile.  Every rotation difference is then exactly 30 b and lands in
bin b (30 b * (1 / 30) rounds to b in float for b < 30), so which bins fill, and how full, is the profile's choice:

  one    b = 2 always                      one bin: the check removes nothing
  tail   b in {1, 5, 9}, p .94 .03 .03     second and third below a tenth of the first: one bin survives (the first 0.1 * max1 cut)
  third  b in {1, 5, 9}, p .55 .42 .03     only the third below a tenth: two bins survive (the second cut)
  four   b in {1, 5, 9, 11}, equal         more than three filled bins: three survive; ties for second / third place occur
  empty  no match at all                   an all-zero histogram

SEEDS holds, per matcher, the seeds for which test_rotation_cases.py found all of that to hold at N keypoints per side."""
import numpy as np
import oracle_match_bind as om
from oracle_bind import KP_DTYPE

N = 300                              # keypoints per side: the smallest size that fills four bins with ties
BOUNDS = (0.0, 0.0, 640.0, 480.0)
PROFILES = {"one": ((2,), (1.0,)), "tail": ((1, 5, 9), (0.94, 0.03, 0.03)), "third": ((1, 5, 9), (0.55, 0.42, 0.03)),
            "four": ((1, 5, 9, 11), (0.25, 0.25, 0.25, 0.25)), "empty": ((2,), (1.0,))}
SURVIVING_BINS = {"one": 1, "tail": 1, "third": 2, "four": 3}
MATCHERS = ("si", "sbp", "bow", "bow_kf", "tri", "tri_general")
SEEDS = {"si": (0, 1), "sbp": (0, 3), "bow": (0, 1), "bow_kf": (0, 4), "tri": (1, 5), "tri_general": (1, 2)}


def make_si_case(rng, n):
    """SearchForInitialization: two frames of one clustered scene, F2's descriptors drawn from F1's with one bit flipped (the shape of
    test_gpu_match.py's contested-points builder), 90 % of the keypoints at octave 0."""
    def frame(m, cx, cy):
        kp = np.zeros(m, KP_DTYPE)
        kp["x"] = np.clip(rng.normal(cx, 60, m), 1, 638).astype(np.float32)
        kp["y"] = np.clip(rng.normal(cy, 60, m), 1, 478).astype(np.float32)
        kp["octave"] = (rng.uniform(0, 1, m) < 0.1).astype(np.int32)
        return kp
    kpA, kpB = frame(n, 320, 240), frame(n, 325, 238)
    dA = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    src = rng.integers(0, n, n)
    kpB["x"] = np.clip(kpA["x"][src] + rng.normal(0, 6, n), 1, 638).astype(np.float32)
    kpB["y"] = np.clip(kpA["y"][src] + rng.normal(0, 6, n), 1, 478).astype(np.float32)
    dB = dA[src].copy()
    dB[np.arange(n), rng.integers(0, 32, n)] ^= (1 << rng.integers(0, 8, n)).astype(np.uint8)
    return dict(kpA=kpA, dA=dA, kpB=kpB, dB=dB, prev=np.stack([kpA["x"], kpA["y"]], 1))


def make_case(matcher, profile, seed):
    """The builder's case with the profile's angles.  Returns (case, b): b[j] = the bin every match of second-side keypoint j lands in."""
    rng = np.random.default_rng(1000 * MATCHERS.index(matcher) + seed)
    bins, prob = PROFILES[profile]
    b = rng.choice(bins, N, p=prob)
    second = ((360 - 30 * b) % 360).astype(np.float32)
    empty = profile == "empty"
    if matcher == "si":
        c = make_si_case(rng, N)
        c["kpA"]["angle"] = 0; c["kpB"]["angle"] = second
        if empty:
            c["kpB"]["octave"] = 1                                   # only octave-0 keypoints take part (ORBmatcher.cc:726-728)
    elif matcher == "sbp":
        from test_oracle_match_ba import make_sbp_case
        q, dq, kp, d, ur, tm = make_sbp_case(rng, N, N, False)
        q["angle"] = 0; kp["angle"] = second
        if empty:
            tm[:] = 7                                                # every keypoint holds a map point already (:2037-2039)
        c = (q, dq, kp, d, ur, tm)
    elif matcher in ("bow", "bow_kf"):
        c = om.make_bow_case(rng, N, N, 40)
        c["valid2"] = (rng.random(N) < 0.8).astype(np.uint8)
        c["kp_k"]["angle"] = 0; c["kp_f"]["angle"] = second
        if empty:
            c["nid_f"] = c["nid_f"] * 3 + 2                          # no vocabulary node in common (the keyframe's are 3 k + 100)
    else:
        c = om.make_tri_case(rng, N, N, 60) if matcher == "tri" else om.make_tri_general_case(rng, N, N, "kb8", 60)
        c["kp1"]["angle"] = 0; c["kp2"]["angle"] = second
        if empty:
            c["mp2"][:] = 1                                          # every KF2 keypoint has a map point (:1073)
    return c, b


def oracle(matcher, c, check_ori):
    """(nmatches, match array) of the oracle, in the layout the device entry point writes."""
    if matcher == "si":
        return om.search_for_initialization(c["kpA"], c["dA"], c["kpB"], c["dB"], BOUNDS, c["prev"], 100, 0.9, check_ori)[:2]
    if matcher == "sbp":
        q, dq, kp, d, ur, tm = c
        return om.search_by_projection(q, dq, kp, d, None, BOUNDS, tm, 100, check_ori)
    if matcher == "bow":
        return om.search_by_bow(c, 0.7, check_ori)
    if matcher == "bow_kf":
        return om.search_by_bow_kf(c, 0.75, check_ori)
    if matcher == "tri":
        return om.search_for_triangulation(c, check_ori, True)
    return om.search_for_triangulation_general(c, check_ori)


def matched_second(matcher, m):
    """Second-side keypoints that hold a match in a result array: sbp and bow index their result by the second side."""
    m = np.asarray(m)
    return np.flatnonzero(m >= 0) if matcher in ("sbp", "bow") else m[m >= 0]
