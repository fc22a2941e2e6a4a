"""The seeded inputs of the Hugging Face pin (oracle/hf_pin.py), shared by the CPU test, the fixture generator
(tools/make_hf_fixtures.py -> tests/golden/hf_pin.npz) and the GPU twin, so that all three run the same arrays."""
import os

import numpy as np

from airslam_amd import synth
from oracle import ref_post
from planted import normalised, planted_pair

SP_IMAGES = [(480, 752, 0), (720, 1280, 3)]                 # (h, w, seed) of synth.gabor_image; the path resizes to 512 x 512 (src/plnet.cpp:258)
LG_PAIRS = [(200, 200, 7), (317, 400, 1351), (1, 5, 8)]     # (n0, n1, seed)
SG_PAIRS = [(200, 200, 7), (300, 280, 1180), (1, 3, 6)]
DESC_STRIDE = 2                                             # the fixture keeps the dense descriptors of every second cell row / column (1 MB per image)
# The matchers' fp32 scores depend on which CPU kernels MKL, ATen and oneDNN pick for the host's instruction set (1-2e-4 apart after 9 LightGlue
# layers between two x86 hosts): the fixture check of the first case of each matcher runs on these portable paths, one thread, on both sides
# (tests/golden/hf_pin_portable.npz).
PORTABLE_CPU_ENV = {"ATEN_CPU_CAPABILITY": "default", "MKL_CBWR": "COMPATIBLE,STRICT", "ONEDNN_MAX_CPU_ISA": "SSE41", "OMP_NUM_THREADS": "1",
                    "MKL_NUM_THREADS": "1"}
PORTABLE_KEYS = ["lg_%d_%d_%d" % LG_PAIRS[0], "sg_%d_%d_%d" % SG_PAIRS[0]]


def sp_input(h, w, seed):
    """-> (gray uint8 [h, w], x float32 [512, 512] in [0, 1] = PLNet::process_image, src/plnet.cpp:246-270)"""
    img = synth.gabor_image(h, w, seed)
    x, _, _ = ref_post.process_image(img)
    return img, x


def lg_input(n0, n1, seed):
    f0, f1 = planted_pair(n0, n1, seed)
    a, b = normalised(f0), normalised(f1)                   # scale 0.5: src/point_matcher.cc:58
    return f0, f1, a, b


def sg_input(n0, n1, seed):
    f0, f1 = planted_pair(n0, n1, seed)
    a, b = normalised(f0, scale=0.7), normalised(f1, scale=0.7)
    return f0, f1, a, b


def matcher_scores(keys):
    """{key: scores} for the fixture keys lg_<n0>_<n1>_<seed> / sg_<n0>_<n1>_<seed> (transformers' ports, oracle/hf_pin.py), computed in a
    child process on PORTABLE_CPU_ENV (the libraries read it when they load)"""
    import subprocess
    import sys
    import tempfile
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = f"import sys; sys.path[:0] = [{root!r}, {os.path.join(root, 'tests')!r}]; import hf_cases; hf_cases._matcher_scores_here(sys.argv[1], sys.argv[2:])"
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "scores.npz")
        subprocess.run([sys.executable, "-c", code, out, *keys], env=dict(os.environ, **PORTABLE_CPU_ENV), check=True)
        z = np.load(out)
        return {k: z[k] for k in keys}


def _matcher_scores_here(out, keys):
    import torch
    from airslam_amd import weights
    from oracle import hf_pin
    torch.set_num_threads(1)
    res = {}
    for k in keys:
        kind, n0, n1, seed = k.split("_")
        if kind == "lg":
            _, _, a, b = lg_input(int(n0), int(n1), int(seed))
            res[k] = hf_pin.lightglue_scores(weights.synthetic_lightglue(1234), a[:, 1:3], a[:, 3:], b[:, 1:3], b[:, 3:])
        else:
            _, _, a, b = sg_input(int(n0), int(n1), int(seed))
            res[k] = hf_pin.superglue_scores(weights.synthetic_superglue(1234), a[:, 1:3], a[:, 0], a[:, 3:], b[:, 1:3], b[:, 0], b[:, 3:])
    np.savez(out, **res)
