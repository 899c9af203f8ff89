"""The four small pairs of tests/golden/sim3_opt_golden.npz: how they were made (tools/gen_sim3_golden.py writes the file from the
analytic model's outputs) and where the model's precondition test finds them."""
import synth_sim3 as s

SPECS = [dict(seed=6021, n=16, outliers=2), dict(seed=6002, n=24, outliers=3, no_kp2=0.15, fix_scale=True),
         dict(seed=6003, n=24, outliers=3, neg_z=0.1, kb8=True), dict(seed=6004, n=12, outliers=3)]


def cases():
    return [s.make_pair(**spec) for spec in SPECS]
