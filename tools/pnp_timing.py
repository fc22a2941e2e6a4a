"""Cost of the PnP RANSAC (kernels_pnp.hip): the batch entry on planted problems (B problems x n correspondences x inlier ratio), timed with device
events, next to the host core (pnp_core.h compiled for the host) on one CPU thread over the same problems.  Run it under
`rocprofv3 --kernel-trace --stats` for the per-kernel split.
    python tools/pnp_timing.py [--reps R]        (on an MI355X; one JSON line per measurement)"""
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from airslam_amd import api, weights  # noqa: E402
import pnp_ref as pr  # noqa: E402

SHIM = '#include "pnp_core.h"\nextern "C" int core_pnp(const float* o, const float* i, int n, const double* K, double* T, double* R, uint8_t* m, int* c, int* s) ' \
       '{ return pnp_solve_host(o, i, n, K, T, R, m, c, s); }\n'


def host_core():
    d = tempfile.mkdtemp()
    with open(os.path.join(d, "c.cpp"), "w") as f:
        f.write(SHIM)
    so = os.path.join(d, "libc.so")
    subprocess.run(["g++", "-std=c++17", "-O2", "-w", "-fPIC", "-ffp-contract=off", "-shared", "-I" + os.path.join(ROOT, "airslam_amd", "csrc"),
                    os.path.join(d, "c.cpp"), "-o", so], check=True)
    lib = C.CDLL(so)
    lib.core_pnp.argtypes = [C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 6
    return lib


def main(reps=20):
    import torch
    ctx = api.Context(lightglue=weights.synthetic_lightglue(1234), max_batch=1, max_keypoints=1024)
    core = host_core()
    K = np.array(pr.K_EUROC)
    for B in (1, 8, 64):
        for n in (50, 300, 1000):
            for ratio in (0.9, 0.6, 0.3):
                probs = [pr.planted(n, ratio, seed=1000 * b + n)[:2] for b in range(B)]
                obj = torch.from_numpy(np.stack([p[0] for p in probs])).cuda()
                img = torch.from_numpy(np.stack([p[1] for p in probs])).cuda()
                nn = torch.full((B,), n, dtype=torch.int32, device="cuda")
                Twc = torch.zeros((B, 16), dtype=torch.float64, device="cuda")
                mask = torch.zeros((B, n), dtype=torch.uint8, device="cuda")
                cnt = torch.zeros(B, dtype=torch.int32, device="cuda")
                st = torch.cuda.Stream()                        # a stream of its own: a NULL handle would send the work to the context's stream
                for _ in range(3):
                    ctx.pnp_ransac_batch_dev(obj, img, nn, K, Twc, mask, cnt, stream=st.cuda_stream)
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(st)
                for _ in range(reps):
                    ctx.pnp_ransac_batch_dev(obj, img, nn, K, Twc, mask, cnt, stream=st.cuda_stream)
                e1.record(st)
                torch.cuda.synchronize()
                dev_ms = e0.elapsed_time(e1) / reps
                t0 = time.perf_counter()
                for o, i in probs:
                    T, R, m, c, s = np.zeros(16), np.zeros(12), np.zeros(n, np.uint8), C.c_int(0), np.zeros(100, np.int32)
                    core.core_pnp(o.ctypes.data, i.ctypes.data, n, K.ctypes.data, T.ctypes.data, R.ctypes.data, m.ctypes.data, C.byref(c), s.ctypes.data)
                host_ms = (time.perf_counter() - t0) * 1e3
                print(json.dumps(dict(what="pnp_batch", B=B, n=n, inlier_ratio=ratio, device_ms_per_batch=round(dev_ms, 4),
                                      host_core_ms_one_thread=round(host_ms, 3), count_mean=float(cnt.float().mean()))), flush=True)
    ctx.close()


if __name__ == "__main__":
    main(int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 20)
