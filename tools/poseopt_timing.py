"""Cost of the pose-only frame optimisation (kernels_poseopt.hip) on planted problems (B problems x n constraints x inlier ratio), timed with device
events: the batch entry, the tracking composite (gather + PnP + seed + optimisation), airfe_track_pose_batch_dev on the same inputs (the cost the new
step is added to), and the host core (poseopt_core.h compiled for the host) on ONE CPU thread over the same B problems.  Medians over --reps timed
calls after a warm-up, with the spread (min / max).  Run it under `rocprofv3 --kernel-trace --stats` for the per-kernel split.
    python tools/poseopt_timing.py [--reps R] [--quick]        (on an MI355X; one JSON line per measurement)"""
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
import poseopt_ref as po  # noqa: E402

SHIM = '#include "poseopt_core.h"\nextern "C" int core_poseopt(const double* X, const double* o, int n, const double* cam, const double* Tcb, ' \
       'const double* thr, const double* T0, double* T, double* R, uint8_t* m, int* c) ' \
       '{ return poseopt_solve_host(X, o, n, cam, Tcb, thr, T0, T, R, m, c, nullptr); }\n'


def host_core():
    d = tempfile.mkdtemp()
    with open(os.path.join(d, "c.cpp"), "w") as f:
        f.write(SHIM)
    so = os.path.join(d, "libc.so")
    subprocess.run(["g++", "-std=c++17", "-O2", "-w", "-fPIC", "-ffp-contract=off", "-shared", "-I" + os.path.join(ROOT, "airslam_amd", "csrc"),
                    os.path.join(d, "c.cpp"), "-o", so], check=True)
    lib = C.CDLL(so)
    lib.core_poseopt.argtypes = [C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 8
    return lib


def timed(fn, st, reps, warm=3):
    """per-call device milliseconds of fn() on stream st: (median, min, max) over reps calls, each between its own pair of events"""
    import torch
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record(st)
        fn()
        b.record(st)
    torch.cuda.synchronize()
    ms = sorted(a.elapsed_time(b) for a, b in ev)
    return round(float(np.median(ms)), 4), round(ms[0], 4), round(ms[-1], 4)


def main(reps=20, quick=False):
    import torch
    ctx = api.Context(lightglue=weights.synthetic_lightglue(1234), max_batch=1, max_keypoints=1024)
    core = host_core()
    cam, thr, K = np.array(po.CAM_EUROC), np.array(po.THR_EUROC), np.array(pr.K_EUROC)
    eye = np.eye(4).reshape(16)
    for B in ((64,) if quick else (1, 8, 64)):
        for n in (100, 300, 1024):
            for ratio in (0.9, 0.5):
                probs = [po.planted_constraints(n, ratio, seed=1000 * b + n)[:2] for b in range(B)]
                X = torch.from_numpy(np.stack([p[0] for p in probs])).cuda()
                obs = torch.from_numpy(np.stack([p[1] for p in probs])).cuda()
                nn = torch.full((B,), n, dtype=torch.int32, device="cuda")
                T0 = torch.from_numpy(np.tile(eye, (B, 1))).cuda()
                Twc = torch.zeros((B, 16), dtype=torch.float64, device="cuda")
                mask = torch.zeros((B, n), dtype=torch.uint8, device="cuda")
                num = torch.zeros(B, dtype=torch.int32, device="cuda")
                ok = torch.zeros(B, dtype=torch.int32, device="cuda")
                st = torch.cuda.Stream()                        # a stream of its own: a NULL handle would send the work to the context's stream
                # the composite's inputs: keyframe points, current rows (row i sees point i), the identity list
                feat = torch.zeros((B, n, 259))
                feat[:, :, 1:3] = torch.from_numpy(np.stack([p[1][:, :2] for p in probs]).astype(np.float32))
                feat = feat.cuda()
                tidx = torch.from_numpy(np.tile(np.stack([np.arange(n), np.arange(n)], 1).astype(np.int32), (B, 1, 1))).cuda()
                opt = timed(lambda: ctx.frame_optimize_batch_dev(X, obs, nn, T0, cam, thr, Twc, mask, num, stream=st.cuda_stream), st, reps)
                inl = float(num.float().mean())
                comp = timed(lambda: ctx.track_pose_opt_batch_dev(cam, thr, 50, X, feat, tidx, nn, Twc, mask, num, ok, stream=st.cuda_stream), st, reps)
                pnp = timed(lambda: ctx.track_pose_batch_dev(K, X, feat, tidx, nn, Twc, mask, num, stream=st.cuda_stream), st, reps)
                host = []
                for _ in range(3):
                    t0 = time.perf_counter()
                    for x, o in probs:
                        T, R, m, c = np.zeros(16), np.zeros(12), np.zeros(n, np.uint8), C.c_int(0)
                        core.core_poseopt(x.ctypes.data, o.ctypes.data, n, cam.ctypes.data, None, thr.ctypes.data, eye.ctypes.data, T.ctypes.data,
                                          R.ctypes.data, m.ctypes.data, C.byref(c))
                    host.append((time.perf_counter() - t0) * 1e3)
                print(json.dumps(dict(what="poseopt", B=B, n=n, inlier_ratio=ratio, reps=reps, batch_ms_median_min_max=opt, composite_ms_median_min_max=comp,
                                      track_pose_ms_median_min_max=pnp, host_core_ms_one_thread_median=round(float(np.median(host)), 3),
                                      host_core_ms_min_max=(round(min(host), 3), round(max(host), 3)), num_inliers_mean=inl)), flush=True)
    ctx.close()


if __name__ == "__main__":
    main(int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 20, "--quick" in sys.argv)
