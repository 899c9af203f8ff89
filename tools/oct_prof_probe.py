"""GPU-box probe (debug build: make EXTRA=-DOCT_PROF): shader cycles of the octree kernel's phases for workgroup 0 (level 0 of frame 0).
The form is the one the extractor reserves with (ORBHIP_OCTREE=iterative: k_octree, else k_octree_tab); prints one JSON line per run."""
import ctypes as C, json, sys, os
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "orb-slam3-mac_amd", "python"))
import numpy as np, torch, orbhip
B, W, H = 256, 640, 480
ctx = orbhip.Context(0); ext = orbhip.Extractor(ctx, 1000, 1.2, 8, 20, 7); ext.reserve(W, H, B)
imgs = torch.from_numpy(orbhip.synth_frames(W, H, B, seed=7)).cuda()
buf = (C.c_longlong * 8)()
iterative = os.environ.get("ORBHIP_OCTREE") == "iterative" or not hasattr(orbhip.lib, "orbhip_debug_octree")
names = ["gather", "roots", "subdivision", "best", "output+perm"] if iterative else ["gather", "paths+tables", "stop+list+final+lookup", "best", "output+perm"]
for it in range(2):
    orbhip.lib.orbhip_debug_oct_prof(buf, 1)
    ext.extract_device(imgs.data_ptr(), W, H, W, W * H, B, (0, 0)); ctx.synchronize()
    orbhip.lib.orbhip_debug_oct_prof(buf, 0)
    v = list(buf)
    d = {"form": "iterative" if iterative else "table", "cycles": dict(zip(names, v[:5])), "total": sum(v[:5]), "passes": v[5]}
    print(json.dumps(d))
