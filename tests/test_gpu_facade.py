"""The reference's OWN façade — the reference's src/feature_detector.cc and src/point_matcher.cc, compiled unchanged (shim/Makefile) — running
on the GPU through the TensorRT-free wrappers and libairfe.so (missing #2: INTEGRATION.md's "compile untouched" as a tested
statement).  oracle/_ref/facade_gpu is built where the reference tree is (oracle/Makefile, __graft_entry__.build()) and is used as it is elsewhere.
Configuration goes through the reference's own include/read_configs.h (a YAML file in its format); every output of all six Detect overloads
(src/feature_detector.cc:36,52,62,71,83,97) and of MatchingPoints (src/point_matcher.cc:50-107) must equal, byte for byte, what the ctypes path
returns through the same C ABI with the same packs."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from airslam_amd import api, synth, weights
from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu
EXE = os.path.join(ROOT, "oracle", "_ref", "facade_gpu")

YAML = """plnet:
  use_superpoint: {sp}
  max_keypoints: 400
  keypoint_threshold: 0.004
  remove_borders: 4 
  line_threshold: 0.5
  line_length_threshold: 20

point_matcher:
  matcher: {m}   # 0 for lightglue, 1 for superglue
  image_width: 752
  image_height: 480
  onnx_file: "{onnx}"
  engine_file: "{eng}"

keyframe:
  min_init_stereo_feature: 90
  lost_num_match: 10
  min_num_match: 30
  max_num_match: 80
  tracking_point_rate: 0.65  
  tracking_parallax_rate: 0.1

optimization:
  tracking:
    mono_point: 50
    stereo_point: 75
    mono_line: 50
    stereo_line: 75
    rate: 0.5
  backend:
    mono_point: 50
    stereo_point: 75
    mono_line: 50
    stereo_line: 75
    rate: 0.5

ros_publisher:
  feature: 1
  feature_topic: "/AirSLAM/feature"
  frame_pose: 1
  frame_pose_topic: "/AirSLAM/frame_pose"
  frame_odometry_topic: "/AirSLAM/LatestOdometry"
  keyframe: 1
  keyframe_topic: "/AirSLAM/keyframe"
  path_topic: "/AirSLAM/odometry"
  map: 1
  map_topic: "/AirSLAM/map"
  mapline: 1
  mapline_topic: "/AirSLAM/mapline"
  reloc: 0
  reloc_topic: "/AirSLAM/reloc"
"""


@pytest.fixture(scope="module")
def models(tmp_path_factory):
    if not os.path.exists(EXE):
        pytest.skip("oracle/_ref/facade_gpu was not built (no reference tree where the tree was built and no prebuilt binary)")
    md = tmp_path_factory.mktemp("models")
    w = dict(sp=weights.synthetic_superpoint(1234), s0=weights.synthetic_plnet_s0(1234), lg=weights.synthetic_lightglue(1234),
             sg=weights.synthetic_superglue(1234))
    weights.save_pack(str(md / "superpoint_v1_sim_int32.airfe"), w["sp"])
    weights.save_pack(str(md / "plnet_s0.airfe"), w["s0"])
    shutil.copy(os.path.join(GOLDEN, "plnet_s1.airfe"), str(md / "plnet_s1.airfe"))
    weights.save_pack(str(md / "superpoint_lightglue.airfe"), w["lg"])
    weights.save_pack(str(md / "superglue_outdoor_sim_int32.airfe"), w["sg"])
    left, right = synth.stereo_pair(480, 752, 4)
    left.tofile(str(md / "l.raw")); right.tofile(str(md / "r.raw"))
    return md, w, left, right


@pytest.mark.parametrize("use_sp,matcher", [(1, 0), (0, 0), (0, 1)])
def test_reference_facade_on_the_gpu_equals_the_c_abi(models, tmp_path, use_sp, matcher):
    md, w, left, right = models
    od = tmp_path / "out"; od.mkdir()
    onnx = "superglue_outdoor_sim_int32.onnx" if matcher else "superpoint_lightglue.onnx"
    (tmp_path / "vo.yaml").write_text(YAML.format(sp=use_sp, m=matcher, onnx=onnx, eng=onnx.replace(".onnx", ".engine")))
    r = subprocess.run([EXE, str(tmp_path / "vo.yaml"), str(md), str(md / "l.raw"), str(md / "r.raw"), "480", "752", str(od)],
                       capture_output=True, text=True)
    assert r.returncode == 0, f"rc={r.returncode}\n{r.stdout}\n{r.stderr}"
    print(r.stdout)
    assert "Failed when extracting point features" in r.stdout            # the empty-image call prints the reference's message

    def rd(name, dt, cols=None):
        a = np.fromfile(str(od / name), dtype=dt)
        return a.reshape(-1, cols) if cols else a

    s1 = os.path.join(GOLDEN, "plnet_s1.airfe")
    pl = api.Context(superpoint=w["s0"], plnet_s1=s1, max_batch=1, enc_chunk=1, line_threshold=0.5, line_length_threshold=20.0)
    pfl, pll, pjl = pl.detect_plnet(left, None, want_junctions=True)
    pfr, plr, _ = pl.detect_plnet(right, None, want_junctions=False)
    pl.close()
    assert len(pll) >= 30 and len(pjl) >= 20 and len(pfl) >= 100
    if use_sp:
        sp = api.Context(superpoint=w["sp"], max_batch=1, enc_chunk=1)
        fl, fr = sp.detect_points(left), sp.detect_points(right)
        sp.close()
    else:
        fl, fr = pfl, pfr
    eq = np.testing.assert_array_equal
    eq(rd("d0_feat.bin", np.float32, 259), fl)                         # Detect(image, features): SuperPoint if use_superpoint else PLNet
    eq(rd("d1_feat.bin", np.float32, 259), pfl); eq(rd("d1_lines.bin", np.float64, 4), pll)
    eq(rd("d2_feat.bin", np.float32, 259), pfl); eq(rd("d2_lines.bin", np.float64, 4), pll); eq(rd("d2_junc.bin", np.float32, 259), pjl)
    eq(rd("d3_featl.bin", np.float32, 259), fl); eq(rd("d3_featr.bin", np.float32, 259), fr)
    eq(rd("d4_featl.bin", np.float32, 259), pfl); eq(rd("d4_featr.bin", np.float32, 259), pfr)
    eq(rd("d4_linesl.bin", np.float64, 4), pll); eq(rd("d4_linesr.bin", np.float64, 4), plr)
    eq(rd("d5_featl.bin", np.float32, 259), pfl); eq(rd("d5_featr.bin", np.float32, 259), pfr)
    eq(rd("d5_linesl.bin", np.float64, 4), pll); eq(rd("d5_linesr.bin", np.float64, 4), plr)
    eq(rd("d5_junc.bin", np.float32, 259), pjl)                        # junctions of the LEFT image only (src/feature_detector.cc:100-101)
    # MatchingPoints on the features of overload 3, NormalizeKeypoints + bottomRows(258) evaluated by the reference's own code
    c = api.Context(lightglue=w["lg"], max_batch=1, max_keypoints=1024) if matcher == 0 else \
        api.Context(superglue=w["sg"], matcher=1, max_batch=1, max_keypoints=1024)
    pm = api.PointMatcher(c, 752, 480, matcher)
    cnt, matches = pm.MatchingPoints(np.asfortranarray(fl.T), np.asfortranarray(fr.T))
    c.close()
    assert cnt >= 50
    eq(rd("m_query.bin", np.int32), np.array([m[0] for m in matches], np.int32))
    eq(rd("m_train.bin", np.int32), np.array([m[1] for m in matches], np.int32))
    eq(rd("m_dist.bin", np.float32), np.array([m[2] for m in matches], np.float32))
    if not use_sp and matcher == 0:
        # the one-call keyframe class (shim/include/airfe_keyframe.h) == the two facade calls it stands for.  (The facade's matcher context is built for
        # 1024 keypoints, the keyframe's for max_keypoints = 400: the arena size does not enter the arithmetic.)
        eq(rd("k_featl.bin", np.float32, 259), pfl); eq(rd("k_featr.bin", np.float32, 259), pfr)
        eq(rd("k_linesl.bin", np.float64, 4), pll); eq(rd("k_linesr.bin", np.float64, 4), plr)
        eq(rd("k_junc.bin", np.float32, 259), pjl)
        eq(rd("k_query.bin", np.int32), rd("m_query.bin", np.int32))
        eq(rd("k_train.bin", np.int32), rd("m_train.bin", np.int32))
        eq(rd("k_dist.bin", np.float32), rd("m_dist.bin", np.float32))
        # the temporal match riding in the keyframe's forward == the facade's own MatchingPoints(last keyframe, left) on the same features
        assert len(rd("t_query.bin", np.int32)) >= 50
        eq(rd("t_query.bin", np.int32), rd("tr_query.bin", np.int32))
        eq(rd("t_train.bin", np.int32), rd("tr_train.bin", np.int32))
        eq(rd("t_dist.bin", np.float32), rd("tr_dist.bin", np.float32))
