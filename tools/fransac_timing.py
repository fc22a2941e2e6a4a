"""Cost of the F-matrix RANSAC (kernels_fransac.hip): the batch entry alone on planted lists (B pairs x K matches x inlier ratio; run it under
`rocprofv3 --kernel-trace --stats` for the per-kernel split), and the sequence driver's frames/s with outlier rejection off and on (S = 8, 32).
    python tools/fransac_timing.py [--kernels] [--seq]        (on an MI355X; one JSON line per measurement)"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from airslam_amd import api, seq, synth, weights  # noqa: E402
import fransac_ref as fr  # noqa: E402


def kernels(reps=20):
    import torch
    ctx = api.Context(lightglue=weights.synthetic_lightglue(1234), max_batch=1, max_keypoints=1024)
    for B in (32, 64):
        for K in (400, 1024):
            for ratio in (0.9, 0.6, 0.3):
                f0 = torch.zeros((B, K, 259)); f1 = torch.zeros_like(f0)
                idx = torch.zeros((B, K, 2), dtype=torch.int32); sc = torch.zeros((B, K))
                for b in range(B):
                    _, _, _, xyf = fr.planted(K, ratio, seed=b)
                    a0, a1 = fr.features_for(xyf, seed=b)
                    f0[b] = torch.from_numpy(a0); f1[b] = torch.from_numpy(a1)
                    idx[b, :, 0] = idx[b, :, 1] = torch.arange(K, dtype=torch.int32)
                f0, f1, idx, sc = f0.cuda(), f1.cuda(), idx.cuda(), sc.cuda()
                nm0 = torch.full((B,), K, dtype=torch.int32, device="cuda")
                work = [(idx.clone(), nm0.clone()) for _ in range(reps + 2)]
                for i in range(2):
                    ctx.fundamental_ransac_batch_dev(f0, f1, work[i][0], sc, work[i][1])
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for i in range(2, reps + 2):
                    ctx.fundamental_ransac_batch_dev(f0, f1, work[i][0], sc, work[i][1])
                e1.record(); torch.cuda.synchronize()
                kept = float(work[-1][1].float().mean())
                print(json.dumps(dict(what="fransac_batch", B=B, K=K, inlier_ratio=ratio, us_per_call=e0.elapsed_time(e1) / reps * 1e3, kept_mean=kept)), flush=True)
    ctx.close()


def sequences(N=40):
    import torch
    W, H = 752, 480
    s1 = os.path.join(ROOT, "tests", "golden", "plnet_s1.airfe")
    lg = weights.synthetic_lightglue(1234)
    cfg = seq.KeyframeConfig(tracking_point_rate=0.2, min_init_stereo_feature=60, min_num_match=100, max_num_match=110)
    for S in (8, 32):
        frames = [list(synth.stereo_sequence(N, H, W, 40 + s, scene_len=13)) for s in range(S)]
        Ls = [torch.from_numpy(np.stack([frames[s][t][0] for s in range(S)])).cuda() for t in range(N)]
        Rs = [torch.from_numpy(np.stack([frames[s][t][1] for s in range(S)])).cuda() for t in range(N)]
        for on in (False, True):
            common = dict(max_keypoints=400, image_width=W, image_height=H, precision=1, matcher_precision=1)
            kf = api.Context(superpoint=weights.synthetic_plnet_s0(1234), plnet_s1=s1, lightglue=lg, max_batch=S, enc_chunk=min(2 * S, 64), **common)
            nf = api.Context(superpoint=weights.synthetic_superpoint(1234), lightglue=lg, max_batch=S, enc_chunk=min(S, 64), **common)
            ns = seq.NativeSequences(kf, nf, S, cfg, copy_results=False, outlier_rejection=on)
            for t in range(4):
                ns.step(Ls[t], Rs[t])
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            kfs = 0
            for t in range(4, N):
                kfs += sum(r.frame_type != seq.NORMAL for r in ns.step(Ls[t], Rs[t]))
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            ns.close(); kf.close(); nf.close()
            print(json.dumps(dict(what="seq_native", S=S, outlier_rejection=on, steps=N - 4, ms_per_step=dt / (N - 4) * 1e3, frames_per_s=S * (N - 4) / dt,
                                  keyframes=int(kfs))), flush=True)


if __name__ == "__main__":
    if "--kernels" in sys.argv or len(sys.argv) == 1:
        kernels()
    if "--seq" in sys.argv or len(sys.argv) == 1:
        sequences()
