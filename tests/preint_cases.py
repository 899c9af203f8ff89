"""Inputs of the preintegration tests: synthetic 200 Hz chains, the chain lengths and batch shapes at which the two device forms take
another path (the wave form works through 64 measurements at a time, the lane form through 64 chains per workgroup), a full symmetric
Nga, the branch of IntegratedRotation on both sides of 1e-4, and the longdouble / float32 model results, computed once per case."""
import functools
import numpy as np
import preint_model as pm

F32 = np.float32
LENGTHS = (0, 1, 2, 63, 64, 65, 127, 128, 129, 257, 2000)
BATCHES = (1, 63, 64, 65, 130)
# The information check asks of its inputs that no eigenvalue of C(0:9, 0:9) lies within a factor 8 of the cut 9e-7 * wmax (a change
# at rounding level must not flip a dropped direction).  At 200 Hz a chain of 2 measurements has its position block at 7.0 x the cut
# and one of 2000 its rotation block at 3.3 x: for that check those two lengths are sampled at 100 Hz (28 x) and 1000 Hz (1293 x);
# chains of length 2 inside the ragged batches are at 100 Hz throughout.  Every other length is above 18 x at 200 Hz, length 1 has its
# three exactly singular directions at 0.  test_preint_model.py asserts the condition on the float32 model's covariances.
INFO_DT = {2: 0.01, 2000: 0.001}
NG, NA, NGW, NAW = 1.7e-4, 2.0e-3, 1.9393e-5, 3.0e-3          # EuRoC's IMU.NoiseGyro / NoiseAcc / GyroWalk / AccWalk


def calib_nga(ng=NG, na=NA):
    """IMU::Calib::Set (src/ImuTypes.cc:492-500): diag(ng^2 x 3, na^2 x 3) in float."""
    ng2, na2 = F32(ng) * F32(ng), F32(na) * F32(na)
    return np.diag(np.array([ng2] * 3 + [na2] * 3, F32))


def full_nga(seed=5):
    """A full symmetric positive definite 6 x 6 of the diagonal one's size."""
    rng = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(rng.standard_normal((6, 6)))
    d = np.array([NG ** 2, 2 * NG ** 2, 3 * NG ** 2, NA ** 2, 2 * NA ** 2, 0.5 * NA ** 2])
    s = np.sqrt(d)
    M = (Q * np.array([1.0, 0.7, 0.5, 0.9, 0.6, 0.8])) @ Q.T        # a correlation-like SPD matrix
    M = M * s[:, None] * s[None, :]
    M = ((M + M.T) / 2).astype(F32)
    return ((M + M.T) / F32(2)).astype(F32)


def chain(n, seed, dt=0.005):
    """n measurements (ax, ay, az, wx, wy, wz, dt) of a hand-held motion at 1 / dt Hz, float32."""
    rng = np.random.default_rng(1000 + seed)
    t = np.arange(n) * dt
    ph = rng.uniform(0, 2 * np.pi, 6)
    fr = rng.uniform(0.3, 2.0, 6)
    amp_w, amp_a = rng.uniform(0.1, 0.6, 3), rng.uniform(0.3, 1.5, 3)
    w = amp_w[None, :] * np.sin(2 * np.pi * fr[None, :3] * t[:, None] + ph[None, :3]) + 0.01 * rng.standard_normal((n, 3))
    a = np.array([0.3, 9.7, -0.8])[None, :] + amp_a[None, :] * np.sin(2 * np.pi * fr[None, 3:] * t[:, None] + ph[None, 3:]) + 0.05 * rng.standard_normal((n, 3))
    m = np.zeros((n, 7), F32)
    m[:, 0:3] = a; m[:, 3:6] = w; m[:, 6] = dt * (1 + 0.02 * rng.standard_normal(n))
    return m


def bias(seed):
    rng = np.random.default_rng(2000 + seed)
    return np.concatenate([0.02 * rng.standard_normal(3), 0.1 * rng.standard_normal(3)]).astype(F32)      # bg, ba


def ragged_lengths(B, seed):
    """Lengths of a batch: empty chains first, last and in the middle, lengths on both sides of the wave form's 64."""
    rng = np.random.default_rng(3000 + seed + B)
    if B == 1:
        return [37]
    L = rng.integers(1, 40, B)
    for i, v in zip(range(2, B, 9), (63, 64, 65, 70, 1, 2, 129, 66)):
        L[i] = v
    L[0] = 0; L[B - 1] = 0; L[B // 2] = 0
    return [int(v) for v in L]


def batch(B, seed=0):
    L = ragged_lengths(B, seed)
    return [bias(seed + 7 * c) for c in range(B)], [chain(n, seed + 13 * c, dt=0.01 if n == 2 else 0.005) for c, n in enumerate(L)]


def branch_chain():
    """|w - bg| dt of 0, 0.9e-4 and 1.1e-4 among ordinary measurements: both sides of IntegratedRotation's d < 1e-4."""
    b = bias(77)
    m = chain(12, 77)
    dt = F32(0.005)
    m[:, 6] = dt
    m[3, 3:6] = b[0:3]
    m[6, 3:6] = b[0:3] + np.array([0.9e-4 / 0.005, 0, 0], F32)
    m[9, 3:6] = b[0:3] + np.array([0, 1.1e-4 / 0.005, 0], F32)
    return b, m


def acc_equals_bias_chain(n=20):
    b = bias(78)
    m = chain(n, 78)
    m[:, 0:3] = b[3:6]
    return b, m


@functools.lru_cache(maxsize=None)
def single(n):
    """(bias [1][6], [meas]) of the single-chain case of length n."""
    return [bias(n)], [chain(n, n)]


def info_lengths():
    """(bias list, meas list): one chain of every length of LENGTHS but 0 (C = 0 there), sampled as INFO_DT says."""
    lens = [n for n in LENGTHS if n > 0]
    return [bias(n) for n in lens], [chain(n, n, dt=INFO_DT.get(n, 0.005)) for n in lens]


def models(biases, meas, nga, walk):
    """(longdouble fields, float32 fields) of the chains."""
    return pm.integrate(biases, meas, nga, walk, pm.LD), pm.integrate(biases, meas, nga, walk, F32)


def k_rule_ratios(dev, ref, f32):
    """Per field group: (e_device, e_float32_model, floor = 2^-24 max|group|) over all chains of the batch, taken per chain and the
    worst ratio kept -> name -> (e_dev, e_f32, floor) of the chain with the largest e_dev / (e_f32 + floor)."""
    gd, gr, gf = pm.groups(dev), pm.groups(ref), pm.groups(f32)
    out = {}
    for name in gr:
        B = len(gr[name])
        r = gr[name].reshape(B, -1)
        ed = np.max(np.abs(gd[name].reshape(B, -1).astype(pm.LD) - r), axis=1, initial=0)
        ef = np.max(np.abs(gf[name].reshape(B, -1).astype(pm.LD) - r), axis=1, initial=0)
        fl = np.max(np.abs(r), axis=1, initial=0) * pm.LD(2.0 ** -24)
        with np.errstate(all="ignore"):
            ratio = np.where(ed == 0, 0, ed / (ef + fl))
        i = int(np.argmax(ratio)) if B else 0
        out[name] = (float(ed[i]), float(ef[i]), float(fl[i])) if B else (0.0, 0.0, 0.0)
    return out
