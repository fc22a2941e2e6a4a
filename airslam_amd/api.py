"""Host-side mirror of the reference's front-end interface on top of the libairfe.so C ABI.

`FeatureDetector.Detect` and `PointMatcher.MatchingPoints` keep the names, argument meaning and error behaviour
of include/feature_detector.h:8-31 and include/point_matcher.h:8-24 (bool / match-count returns, printed
messages, early-outs); feature matrices are numpy [259, N] float32 in the reference's Eigen orientation
(column = keypoint), stored Fortran-contiguous so they are byte-identical to Eigen's column-major buffer.

torch is used only as plumbing for the device-resident batch entry points (`Context.*_dev`).
"""
from __future__ import annotations

import ctypes as C
import os
import tempfile
from typing import Dict, Optional

import numpy as np

from . import _lib, weights as W

FEAT = 259


def _pack_arg(x, tmpfiles) -> Optional[bytes]:
    if x is None:
        return None
    if isinstance(x, (str, bytes, os.PathLike)):
        return os.fsencode(x)
    f = tempfile.NamedTemporaryFile(suffix=".airfe", delete=False)
    f.close()
    W.save_pack(f.name, x)
    tmpfiles.append(f.name)
    return f.name.encode()


class AirfeError(RuntimeError):
    pass


def conv_tile_order(order: int) -> int:
    """Tile order of the persistent conv kernels, process-wide (airfe_debug_conv_order): bit 0 conv64r, bit 1 conv128r; set = XCD-blocked walk, cout passes in one
    launch; 0 = raster walk, one launch per pass; -1 = the library's default.  Returns the value before the call.  The same output bytes either way."""
    prev = C.c_int()
    if _lib.lib().airfe_debug_conv_order(int(order), C.byref(prev)) != 0:
        raise AirfeError((_lib.lib().airfe_last_error(None) or b"airfe_debug_conv_order failed").decode())
    return prev.value


class Context:
    """One airfe_ctx: one device, one stream, one calling thread."""

    def __init__(self, superpoint=None, lightglue=None, superglue=None, plnet_s1=None, tuning=None, **cfg):
        """cfg: airfe_cfg fields; tuning: dict of airfe_tuning fields (kernel-selection overrides for A/B runs and tests; the library reads no environment)."""
        self._l = _lib.lib()
        c = _lib.Cfg()
        self._l.airfe_default_cfg(C.byref(c))
        t = None
        if tuning and "conv_order" in tuning:
            # not an airfe_tuning field (the struct's size is pinned): the conv kernels' tile order is one process-wide switch (airfe_debug_conv_order)
            tuning = dict(tuning)
            conv_tile_order(int(tuning.pop("conv_order")))
        if tuning:
            t = _lib.Tuning()
            self._l.airfe_default_tuning(C.byref(t))
            for k, v in tuning.items():
                if k == "reserved" or not hasattr(t, k):
                    raise TypeError(f"unknown airfe_tuning field {k!r}")
                setattr(t, k, int(v))
            c.tuning = C.pointer(t)
        for k, v in cfg.items():
            if not hasattr(c, k):
                raise TypeError(f"unknown airfe_cfg field {k!r}")
            setattr(c, k, v)
        tmp = []
        try:
            c.superpoint_pack = _pack_arg(superpoint, tmp)
            c.lightglue_pack = _pack_arg(lightglue, tmp)
            c.superglue_pack = _pack_arg(superglue, tmp)
            c.plnet_s1_pack = _pack_arg(plnet_s1, tmp)
            h = C.c_void_p()
            rc = self._l.airfe_create(C.byref(c), C.byref(h))
            if rc != 0:
                raise AirfeError((self._l.airfe_last_error(None) or b"airfe_create failed").decode())
        finally:
            for t in tmp:
                os.unlink(t)
        self._h = h
        c.tuning = None                # (read by airfe_create only)
        self.cfg = c
        self.max_keypoints = c.max_keypoints
        self.np_rows = (c.max_keypoints + 15) // 16 * 16

    def close(self):
        if getattr(self, "_h", None):
            self._l.airfe_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc, what):
        if rc != 0:
            raise AirfeError(f"{what}: {(self._l.airfe_last_error(self._h) or b'').decode()}")

    @staticmethod
    def _image(img, wrong_type=None):
        """The 2-D uint8 image check of every host entry -> the array the C entry reads: the caller's, or a contiguous copy where its strides cannot be handed over.
        wrong_type: what a non-image raises (default: AirfeError("empty image"), as an empty one does)."""
        img = np.asarray(img)
        if img.ndim != 2 or img.dtype != np.uint8:
            raise wrong_type if wrong_type is not None else AirfeError("empty image")
        if img.size == 0:
            raise AirfeError("empty image")
        if img.strides[1] != 1 or img.strides[0] < img.shape[1]:      # negative / overlapping row strides: hand over a copy
            img = np.ascontiguousarray(img)
        return img

    # ---------------------------------------------------------------- host, batch-1 (≙ reference infer())
    def detect_points(self, gray: np.ndarray) -> np.ndarray:
        """-> [n, 259] float32 rows (score, x, y, desc).  Raises on an empty image."""
        gray = self._image(gray, TypeError("expected a 2-D uint8 image"))
        cap = self.np_rows
        feat = np.empty((cap, FEAT), dtype=np.float32)
        n = C.c_int(0)
        self._chk(self._l.airfe_detect_points(self._h, gray.ctypes.data, gray.shape[0], gray.shape[1], gray.strides[0],
                                              feat.ctypes.data, cap, C.byref(n)), "airfe_detect_points")
        return feat[:n.value].copy()

    def bow_load(self, voc: dict):
        """voc: dict(desc [n,256] f32, first_child [n] i32, n_children [n] i32, word_id [n] i32, weight [n] f64) — weights.synthetic_vocabulary."""
        d = np.ascontiguousarray(voc["desc"], np.float32); fc = np.ascontiguousarray(voc["first_child"], np.int32)
        nc = np.ascontiguousarray(voc["n_children"], np.int32); wi = np.ascontiguousarray(voc["word_id"], np.int32)
        w = np.ascontiguousarray(voc["weight"], np.float64)
        self._chk(self._l.airfe_bow_load(self._h, d.ctypes.data, fc.ctypes.data, nc.ctypes.data, wi.ctypes.data, w.ctypes.data, d.shape[0]),
                  "airfe_bow_load")

    def bow_transform(self, feat_rows: np.ndarray):
        """≙ the per-feature loop of Database::FrameToBow -> (word_of_features [N] uint32 (UINT_MAX = stopped), weights [N] float64)."""
        f = np.ascontiguousarray(feat_rows, np.float32).reshape(-1, FEAT)
        wid = np.empty((f.shape[0],), np.uint32); w = np.empty((f.shape[0],), np.float64)
        self._chk(self._l.airfe_bow_transform(self._h, f.ctypes.data, f.shape[0], wid.ctypes.data, w.ctypes.data), "airfe_bow_transform")
        return wid, w

    def set_rectify_maps(self, side: int, mapx: np.ndarray, mapy: np.ndarray):
        """≙ Camera's cv::initUndistortRectifyMap outputs (_mapl1/_mapl2 = side 0, _mapr1/_mapr2 = side 1): float32 [h, w] maps."""
        mx = np.ascontiguousarray(mapx, np.float32); my = np.ascontiguousarray(mapy, np.float32)
        if mx.shape != my.shape or mx.ndim != 2:
            raise TypeError("maps must be two 2-D arrays of one shape")
        self._chk(self._l.airfe_set_rectify_maps(self._h, side, mx.ctypes.data, my.ctypes.data, mx.shape[0], mx.shape[1]), "airfe_set_rectify_maps")

    def rectify_detect(self, side: int, raw: np.ndarray, detect: bool = True):
        """≙ Camera::UndistortImage + Detect: raw uint8 image -> (rectified uint8 [h, w], features [n, 259] or None)."""
        raw = self._image(raw)
        rect = np.empty(raw.shape, np.uint8)
        cap = self.np_rows
        feat = np.empty((cap, FEAT), np.float32) if detect else None
        n = C.c_int(0)
        self._chk(self._l.airfe_rectify_detect_points(self._h, side, raw.ctypes.data, raw.shape[0], raw.shape[1], raw.strides[0],
                                                      rect.ctypes.data, feat.ctypes.data if detect else None, cap, C.byref(n)),
                  "airfe_rectify_detect_points")
        return rect, (feat[:n.value].copy() if detect else None)

    def match_lightglue(self, f0: np.ndarray, f1: np.ndarray):
        """f0/f1: [n, 258] rows (normalised x, y, desc) -> (idx [k,2] int32, score [k] float32)."""
        f0 = np.ascontiguousarray(f0, dtype=np.float32)
        f1 = np.ascontiguousarray(f1, dtype=np.float32)
        cap = self.np_rows
        idx = np.empty((cap, 2), dtype=np.int32)
        sc = np.empty((cap,), dtype=np.float32)
        n = C.c_int(0)
        self._chk(self._l.airfe_match_lightglue(self._h, f0.ctypes.data, f0.shape[0], f1.ctypes.data, f1.shape[0],
                                                idx.ctypes.data, sc.ctypes.data, cap, C.byref(n)), "airfe_match_lightglue")
        return idx[:n.value].copy(), sc[:n.value].copy()

    def lightglue_scores(self, f0: np.ndarray, f1: np.ndarray) -> np.ndarray:
        f0 = np.ascontiguousarray(f0, dtype=np.float32)
        f1 = np.ascontiguousarray(f1, dtype=np.float32)
        out = np.empty((f0.shape[0], f1.shape[0]), dtype=np.float32)
        self._chk(self._l.airfe_debug_lightglue_scores(self._h, f0.ctypes.data, f0.shape[0], f1.ctypes.data, f1.shape[0],
                                                       out.ctypes.data), "airfe_debug_lightglue_scores")
        return out

    @staticmethod
    def _stage0(s0):
        """dict of numpy arrays (synth.plnet_stage0_lines layout) -> (_lib.Stage0, keep-alive list)"""
        st = _lib.Stage0()
        keep = []
        for name, _ in _lib.Stage0._fields_:
            a = np.ascontiguousarray(s0[name], dtype=np.float32)
            keep.append(a)
            setattr(st, name, a.ctypes.data)
        return st, keep

    def detect_plnet(self, gray: np.ndarray, stage0=None, want_junctions: bool = False, cap_lines: int = 45056,
                     cap_junc: int = 2048):
        """≙ PLNet::infer -> (feat [n,259], lines [L,4] float64, junctions [K,259])."""
        gray = self._image(gray)
        cap = self.np_rows
        feat = np.empty((cap, FEAT), np.float32)
        lines = np.empty((cap_lines, 4), np.float64)
        junc = np.empty((cap_junc, FEAT), np.float32)
        n, nl, nj = C.c_int(0), C.c_int(0), C.c_int(0)
        st, keep = (self._stage0(stage0) if stage0 is not None else (None, None))
        self._chk(self._l.airfe_detect_plnet(self._h, gray.ctypes.data, gray.shape[0], gray.shape[1], gray.strides[0],
                                             C.byref(st) if st is not None else None, feat.ctypes.data, cap, C.byref(n),
                                             lines.ctypes.data, cap_lines, C.byref(nl), junc.ctypes.data, cap_junc,
                                             C.byref(nj), int(want_junctions)), "airfe_detect_plnet")
        return feat[:n.value].copy(), lines[:nl.value].copy(), junc[:nj.value].copy()

    def stereo_keyframe(self, left: np.ndarray, right: np.ndarray, match: bool = True, want_junctions: bool = True, cap_lines: int = 4096,
                        cap_junc: int = 2048, track: bool = False, ref_feat=None, outlier_rejection: bool = False):
        """ONE stereo keyframe in one call (airfe_stereo_keyframe ≙ map_builder.cc:85-86): -> dict(featL, featR [n,259], linesL, linesR [L,4] float64,
        juncL [K,259], idx [m,2] int32, score [m]) — idx / score absent with match=False.  track=True (airfe_stereo_keyframe_tracked): also the temporal
        match of map_builder.cc:96 against the last keyframe's features (`ref_feat` [n,259]: uploaded when given, else the ones on the device) in the SAME
        LightGlue forward -> track_idx [t,2] (reference, left), track_score [t].  outlier_rejection=True: the temporal list passes the F-matrix RANSAC
        on the device (map_builder.cc:96 passes `true`; the stereo list, :86, never does)."""
        if outlier_rejection and not track:
            raise AirfeError("stereo_keyframe: outlier_rejection applies to the temporal match: pass track=True")
        if ref_feat is not None and not track:
            raise AirfeError("stereo_keyframe: ref_feat is the temporal match's reference: pass track=True")
        if track and not match:
            raise AirfeError("stereo_keyframe: track=True needs match=True (the temporal pair rides in the stereo match's forward)")
        imgs = [self._image(g) for g in (left, right)]
        if imgs[0].shape != imgs[1].shape:
            raise AirfeError("stereo_keyframe: left and right images differ in size")
        if imgs[0].strides[0] != imgs[1].strides[0]:      # one row pitch for both: the C entry takes one stride
            imgs = [np.ascontiguousarray(g) for g in imgs]
        # fresh output arrays, filled by the library directly (like the reference's caller-owned Eigen matrices): the slices returned below own them
        cap = self.np_rows
        fl, fr = np.empty((cap, FEAT), np.float32), np.empty((cap, FEAT), np.float32)
        ll, lr = np.empty((cap_lines, 4), np.float64), np.empty((cap_lines, 4), np.float64)
        jl = np.empty((cap_junc if want_junctions else 0, FEAT), np.float32)
        idx, sc = np.empty((cap if match else 0, 2), np.int32), np.empty((cap if match else 0,), np.float32)
        n = (C.c_int * 6)()
        p = lambda i: C.cast(C.byref(n, 4 * i), C.POINTER(C.c_int))
        args = (self._h, imgs[0].ctypes.data, imgs[1].ctypes.data, imgs[0].shape[0], imgs[0].shape[1], imgs[0].strides[0],
                fl.ctypes.data, fr.ctypes.data, cap, p(0), p(1), ll.ctypes.data, lr.ctypes.data, cap_lines, p(2), p(3),
                jl.ctypes.data if want_junctions else None, cap_junc, p(4), idx.ctypes.data if match else None, sc.ctypes.data, cap, p(5))
        if track:
            ref = None if ref_feat is None else np.ascontiguousarray(ref_feat, dtype=np.float32).reshape(-1, FEAT)
            tidx, tsc, nt = np.empty((cap, 2), np.int32), np.empty((cap,), np.float32), C.c_int(0)
            self._chk(self._l.airfe_set_outlier_rejection(self._h, int(outlier_rejection)), "airfe_set_outlier_rejection")
            try:
                self._chk(self._l.airfe_stereo_keyframe_tracked(*args, None if ref is None else ref.ctypes.data, 0 if ref is None else len(ref),
                                                                tidx.ctypes.data, tsc.ctypes.data, C.byref(nt)), "airfe_stereo_keyframe_tracked")
            finally:
                self._l.airfe_set_outlier_rejection(self._h, 0)
        else:
            self._chk(self._l.airfe_stereo_keyframe(*args), "airfe_stereo_keyframe")
        out = dict(featL=fl[:n[0]], featR=fr[:n[1]], linesL=ll[:n[2]], linesR=lr[:n[3]], juncL=jl[:n[4]])
        if match:
            out["idx"], out["score"] = idx[:n[5]], sc[:n[5]]
        if track:
            out["track_idx"], out["track_score"] = tidx[:nt.value], tsc[:nt.value]
        return out

    def track_frame(self, gray: np.ndarray, ref_feat=None, outlier_rejection: bool = False):
        """ONE tracked frame in one call (airfe_track_frame ≙ map_builder.cc:94-101): points of `gray` + LightGlue against the last keyframe's features
        (`ref_feat` [n,259]: uploaded when given, kept on the device when None) -> (feat [n,259], idx [m,2] (reference, new), score [m]).
        outlier_rejection=True: the list passes the F-matrix RANSAC on the device before it comes back (:101 passes `true`)."""
        gray = self._image(gray)
        cap = self.np_rows
        feat, idx, sc = np.empty((cap, FEAT), np.float32), np.empty((cap, 2), np.int32), np.empty((cap,), np.float32)
        n, nm = C.c_int(0), C.c_int(0)
        ref = None if ref_feat is None else np.ascontiguousarray(ref_feat, dtype=np.float32).reshape(-1, FEAT)
        self._chk(self._l.airfe_set_outlier_rejection(self._h, int(outlier_rejection)), "airfe_set_outlier_rejection")
        try:
            self._chk(self._l.airfe_track_frame(self._h, gray.ctypes.data, gray.shape[0], gray.shape[1], gray.strides[0],
                                                None if ref is None else ref.ctypes.data, 0 if ref is None else len(ref), feat.ctypes.data, cap, C.byref(n),
                                                idx.ctypes.data, sc.ctypes.data, cap, C.byref(nm)), "airfe_track_frame")
        finally:
            self._l.airfe_set_outlier_rejection(self._h, 0)
        return feat[:n.value], idx[:nm.value], sc[:nm.value]

    def promote_frame(self, right: np.ndarray):
        """The promotion of map_builder.cc:104-108 for the frame of the last track_frame call (airfe_promote_frame): Detect(right) + MatchingPoints(left, right)
        with the left rows still on the device -> (featR [n,259], idx [m,2] (left, right), score [m])."""
        right = self._image(right)
        cap = self.np_rows
        feat, idx, sc = np.empty((cap, FEAT), np.float32), np.empty((cap, 2), np.int32), np.empty((cap,), np.float32)
        n, nm = C.c_int(0), C.c_int(0)
        self._chk(self._l.airfe_promote_frame(self._h, right.ctypes.data, right.shape[0], right.shape[1], right.strides[0], feat.ctypes.data, cap, C.byref(n),
                                              idx.ctypes.data, sc.ctypes.data, cap, C.byref(nm)), "airfe_promote_frame")
        return feat[:n.value], idx[:nm.value], sc[:nm.value]

    def adopt_reference(self):
        """`_last_keyframe_feature = frame` for a promoted frame: the last track_frame's rows become the reference, on the device (airfe_adopt_reference)."""
        self._chk(self._l.airfe_adopt_reference(self._h), "airfe_adopt_reference")

    def debug_plnet_stage0(self):
        """The on-device stage-0 line branch of the last detected image: dict in synth.plnet_stage0_lines' layout + jloc / joff."""
        n = 3 * 128 * 128
        out = dict(juncs_pred=np.empty((300, 2), np.float32), lines_pred=np.empty((n, 4), np.float32),
                   iskeep=np.empty((1, 3, 128, 128), np.float32), idx_junc_to_end_min=np.empty((1, 3, 128, 128), np.float32),
                   idx_junc_to_end_max=np.empty((1, 3, 128, 128), np.float32), loi_features=np.empty((1, 128, 128, 128), np.float32),
                   loi_features_thin=np.empty((1, 4, 128, 128), np.float32), loi_features_aux=np.empty((1, 4, 128, 128), np.float32),
                   jloc=np.empty((128, 128), np.float32), joff=np.empty((2, 128, 128), np.float32))
        self._chk(self._l.airfe_debug_plnet_stage0(self._h, *[out[k].ctypes.data for k in (
            "juncs_pred", "lines_pred", "iskeep", "idx_junc_to_end_min", "idx_junc_to_end_max", "loi_features",
            "loi_features_thin", "loi_features_aux", "jloc", "joff")]), "airfe_debug_plnet_stage0")
        return out

    def debug_plnet_j2l(self, fast: bool):
        """(iskeep, idx_min, idx_max) [3*128*128] of the last detected image: as the line path computes them (fast) or in full."""
        out = [np.zeros((3 * 128 * 128,), np.float32) for _ in range(3)]
        self._chk(self._l.airfe_debug_plnet_j2l(self._h, 1 if fast else 0, *(o.ctypes.data for o in out)), "airfe_debug_plnet_j2l")
        return tuple(out)

    def debug_plnet_s1(self, stage0, cap: int = 45056):
        st, keep = self._stage0(stage0)
        la = np.empty((cap, 4), np.float32)
        sc = np.empty((cap,), np.float32)
        m2 = C.c_int(0)
        self._chk(self._l.airfe_debug_plnet_s1(self._h, C.byref(st), la.ctypes.data, sc.ctypes.data, cap, C.byref(m2)),
                  "airfe_debug_plnet_s1")
        return la[:m2.value].copy(), sc[:m2.value].copy()

    def debug_plnet_s1_last(self, cap: int = 45056):
        """(lines_adjusted [m2, 4], scores_line [m2]) of image 0 of the last PLNet call, as the device path's stage-1 kernel left them"""
        la = np.empty((cap, 4), np.float32)
        sc = np.empty((cap,), np.float32)
        m2 = C.c_int(0)
        self._chk(self._l.airfe_debug_plnet_s1_last(self._h, la.ctypes.data, sc.ctypes.data, cap, C.byref(m2)), "airfe_debug_plnet_s1_last")
        return la[:m2.value].copy(), sc[:m2.value].copy()

    def debug_wg_prims(self, v, keep, keys, threads: int):
        """csrc/wg_prims.h alone in one workgroup of `threads` threads: v int32 [n], keep 0 / 1 [n], keys uint32 / uint64 [P] ->
        dict(scan [n], pos [n], totals [5] = scan total, kept, block_sum, block_max, block_min, wave [threads / 64, 3] = sum, max, min, sorted [P])."""
        v = np.ascontiguousarray(v, dtype=np.int32)
        keep = np.ascontiguousarray(keep, dtype=np.uint8)
        keys = np.ascontiguousarray(keys)
        assert keys.dtype in (np.uint32, np.uint64) and keep.shape == v.shape
        out = {"scan": np.empty_like(v), "pos": np.empty_like(v), "totals": np.empty((5,), np.int32), "wave": np.empty((threads // 64, 3), np.int32),
               "sorted": np.empty_like(keys)}
        a = _lib.DebugWgPrimsArgs(v.ctypes.data, keep.ctypes.data, v.size, threads, keys.ctypes.data, keys.size, keys.dtype.itemsize, out["scan"].ctypes.data,
                                  out["pos"].ctypes.data,
                                  out["totals"].ctypes.data, out["wave"].ctypes.data, out["sorted"].ctypes.data)
        self._chk(self._l.airfe_debug_wg_prims(self._h, C.byref(a)), "airfe_debug_wg_prims")
        return out

    def match_superglue(self, f0: np.ndarray, f1: np.ndarray):
        """f0/f1: [n, 259] rows (score, normalised x, y, desc) -> (indices0, indices1, mscores0, mscores1)."""
        f0 = np.ascontiguousarray(f0, dtype=np.float32)
        f1 = np.ascontiguousarray(f1, dtype=np.float32)
        i0 = np.empty((f0.shape[0],), np.int32); i1 = np.empty((f1.shape[0],), np.int32)
        m0 = np.empty((f0.shape[0],), np.float64); m1 = np.empty((f1.shape[0],), np.float64)
        self._chk(self._l.airfe_match_superglue(self._h, f0.ctypes.data, f0.shape[0], f1.ctypes.data, f1.shape[0],
                                                i0.ctypes.data, i1.ctypes.data, m0.ctypes.data, m1.ctypes.data),
                  "airfe_match_superglue")
        return i0, i1, m0, m1

    def assign_points_to_lines(self, lines: np.ndarray, feat: np.ndarray):
        """AssignPointsToLines (src/line_processor.cc:68-120).  lines [L,4] float64, feat [N,259] float32 rows ->
        list of L dicts {point index: distance} (ascending index, like the reference's std::map<int,double>)."""
        lines = np.ascontiguousarray(lines, dtype=np.float64).reshape(-1, 4)
        feat = np.ascontiguousarray(feat, dtype=np.float32).reshape(-1, 259)
        L, N = lines.shape[0], feat.shape[0]
        cap = max(L * N, 1)
        row_ptr = np.zeros((L + 1,), np.int32)
        idx = np.empty((cap,), np.int32); dist = np.empty((cap,), np.float64)
        total = C.c_int(0)
        self._chk(self._l.airfe_assign_points_to_lines(self._h, lines.ctypes.data, L, feat.ctypes.data, N, row_ptr.ctypes.data,
                                                       idx.ctypes.data, dist.ctypes.data, cap, C.byref(total)),
                  "airfe_assign_points_to_lines")
        return [dict(zip(idx[row_ptr[i]:row_ptr[i + 1]].tolist(), dist[row_ptr[i]:row_ptr[i + 1]].tolist())) for i in range(L)]

    @staticmethod
    def _relation_csr(relation):
        row_ptr = np.zeros((len(relation) + 1,), np.int32)
        for i, rel in enumerate(relation):
            row_ptr[i + 1] = row_ptr[i] + len(rel)
        idx = np.array([k for rel in relation for k in sorted(rel)], np.int32).reshape(-1)
        return row_ptr, np.ascontiguousarray(idx)

    def match_lines(self, points_on_line0, points_on_line1, point_matches, point_num0: int, point_num1: int):
        """MatchLines (src/line_processor.cc:122-172).  points_on_line{0,1}: the relations returned by assign_points_to_lines;
        point_matches: [(queryIdx, trainIdx), ...] -> list of len(points_on_line0) matched line indices of frame 1 (-1: none)."""
        rp0, pi0 = self._relation_csr(points_on_line0)
        rp1, pi1 = self._relation_csr(points_on_line1)
        m = np.ascontiguousarray(np.array([(int(a), int(b)) for a, b in point_matches], np.int32).reshape(-1, 2))
        out = np.full((max(len(points_on_line0), 1),), -1, np.int32)
        self._chk(self._l.airfe_match_lines(self._h, rp0.ctypes.data, pi0.ctypes.data if pi0.size else None, len(points_on_line0),
                                            int(point_num0), rp1.ctypes.data, pi1.ctypes.data if pi1.size else None,
                                            len(points_on_line1), int(point_num1), m.ctypes.data if m.size else None, m.shape[0],
                                            out.ctypes.data), "airfe_match_lines")
        return out[:len(points_on_line0)].tolist()

    def superglue_scores(self, f0: np.ndarray, f1: np.ndarray) -> np.ndarray:
        f0 = np.ascontiguousarray(f0, dtype=np.float32)
        f1 = np.ascontiguousarray(f1, dtype=np.float32)
        out = np.empty((f0.shape[0] + 1, f1.shape[0] + 1), dtype=np.float32)
        self._chk(self._l.airfe_debug_superglue_scores(self._h, f0.ctypes.data, f0.shape[0], f1.ctypes.data, f1.shape[0],
                                                       out.ctypes.data), "airfe_debug_superglue_scores")
        return out

    def debug_lg_filter(self, scores: np.ndarray):
        """filter_matches alone on a host score matrix [n0, n1] -> (idx [k,2], score [k])."""
        scores = np.ascontiguousarray(scores, dtype=np.float32)
        cap = self.np_rows
        idx = np.empty((cap, 2), np.int32); sc = np.empty((cap,), np.float32)
        n = C.c_int(0)
        self._chk(self._l.airfe_debug_lg_filter(self._h, scores.ctypes.data, scores.shape[0], scores.shape[1], idx.ctypes.data,
                                                sc.ctypes.data, cap, C.byref(n)), "airfe_debug_lg_filter")
        return idx[:n.value].copy(), sc[:n.value].copy()

    def debug_sg_decode(self, z: np.ndarray):
        """SuperGlue decode alone on a host score matrix [n0+1, n1+1] -> (indices0, indices1, mscores0, mscores1)."""
        z = np.ascontiguousarray(z, dtype=np.float32)
        n0, n1 = z.shape[0] - 1, z.shape[1] - 1
        i0 = np.empty((n0,), np.int32); i1 = np.empty((n1,), np.int32)
        m0 = np.empty((n0,), np.float64); m1 = np.empty((n1,), np.float64)
        self._chk(self._l.airfe_debug_sg_decode(self._h, z.ctypes.data, n0, n1, i0.ctypes.data, i1.ctypes.data, m0.ctypes.data,
                                                m1.ctypes.data), "airfe_debug_sg_decode")
        return i0, i1, m0, m1

    def debug_sg_sinkhorn(self, sim_list, alpha: float, iters: int, form: int = 0):
        """launch_sg_sinkhorn alone on a batch of host coupling matrices [n0, n1] (each its own shape) -> ([Z [n0+1, n1+1], ...], form_ran).
        form: 0 the launcher's dispatch, 1 the per-half-iteration kernels, 2 the register-resident kernel (AirfeError where it does not apply);
        form_ran: 1 per-half-iteration, 2 / 3 the register-resident instantiations <13, 7> / <9, 17>."""
        sims = [np.asarray(s, dtype=np.float32) for s in sim_list]
        b = len(sims)
        ld = max(max(s.shape) for s in sims)
        buf = np.full((b, ld, ld), np.nan, np.float32)
        lens = np.empty((b, 2), np.int32)
        for i, s in enumerate(sims):
            buf[i, :s.shape[0], :s.shape[1]] = s
            lens[i] = s.shape
        z = np.full((b, ld + 1, ld + 1), np.nan, np.float32)
        ran = C.c_int(0)
        self._chk(self._l.airfe_debug_sg_sinkhorn(self._h, buf.ctypes.data, lens.ctypes.data, b, ld, float(alpha), int(iters), int(form), z.ctypes.data,
                                                  C.byref(ran)), "airfe_debug_sg_sinkhorn")
        return [z[i, :s.shape[0] + 1, :s.shape[1] + 1].copy() for i, s in enumerate(sims)], ran.value

    def debug_lg_prepare(self, f0, f1, n0, n1, wr, prec, kp_off=1, normalize=None, second=None, slack_rows=0):
        """launch_lg_prepare alone (include/airfe_debug.h, airfe_debug_lg_prepare): f0 / f1 [B, cap, ld] host rows, n0 / n1 [B], wr [32, 2]; normalize = (cx, cy,
        linv) or None; second = (f0x [n0x, ld], f1x [n1x, ld]) with B = 1.  -> dict x32, xb [rows, 256], rot_cos, rot_sin [rows, 32], lens [2 Bt], rows_past, Np;
        rows = 2 Bt Np + slack_rows."""
        f32 = lambda t: np.ascontiguousarray(t, np.float32)
        f0, f1, wr = f32(f0), f32(f1), f32(wr)
        n0, n1 = np.ascontiguousarray(n0, np.int32), np.ascontiguousarray(n1, np.int32)
        b, cap, ld = f0.shape
        bt = 2 if second is not None else b
        rows = 2 * bt * self.np_rows + int(slack_rows)
        out = {"x32": np.empty((rows, 256), np.float32), "xb": np.empty((rows, 256), np.float32), "rot_cos": np.empty((rows, 32), np.float32),
               "rot_sin": np.empty((rows, 32), np.float32), "lens": np.empty((2 * bt,), np.int32)}
        cx, cy, linv = normalize if normalize is not None else (0.0, 0.0, 1.0)
        a = _lib.DebugLgPrepareArgs(prec=prec, B=b, cap=cap, ld=ld, kp_off=kp_off, normalize=int(normalize is not None), cx=cx, cy=cy, linv=linv,
                                    f0=f0.ctypes.data, f1=f1.ctypes.data, n0=n0.ctypes.data, n1=n1.ctypes.data, wr=wr.ctypes.data, slack_rows=int(slack_rows),
                                    rows=rows, **{k: v.ctypes.data for k, v in out.items()})
        if second is not None:
            x0, x1 = f32(second[0]).reshape(-1, ld), f32(second[1]).reshape(-1, ld)
            k0, k1 = np.zeros((max(len(x0), 1), ld), np.float32), np.zeros((max(len(x1), 1), ld), np.float32)      # (an empty side still needs an address)
            k0[:len(x0)], k1[:len(x1)] = x0, x1
            a.f0x, a.f1x, a.n0x, a.n1x = k0.ctypes.data, k1.ctypes.data, len(x0), len(x1)
        self._chk(self._l.airfe_debug_lg_prepare(self._h, C.byref(a)), "airfe_debug_lg_prepare")
        out["rows_past"], out["Np"] = int(a.rows_past), self.np_rows
        return out

    def debug_sg_front(self, f0, f1, n0, n1, prec, split, normalize=0):
        """SuperGlue's front alone (include/airfe_debug.h, airfe_debug_sg_front): f0 / f1 [B, cap, 259] host rows (score, x, y, descriptor), n0 / n1 [B]; prec the
        context's 2-byte type (1 under a fp32 context); split 1 = the keypoint encoder's large layers as GEMMs.  -> dict lens [2B], x32, xb [rows, 256] and, split,
        h128 [rows, 128], hb [rows, 256] (rows = M rounded up to 128, M = 2 B Np), rows_past, Np, M."""
        f0, f1 = np.ascontiguousarray(f0, np.float32), np.ascontiguousarray(f1, np.float32)
        n0, n1 = np.ascontiguousarray(n0, np.int32), np.ascontiguousarray(n1, np.int32)
        b, cap, ld = f0.shape
        assert ld == FEAT and f1.shape == f0.shape and n0.shape == (b,) and n1.shape == (b,)
        m = 2 * b * self.np_rows
        rows = (m + 127) // 128 * 128
        out = {"lens": np.empty((2 * b,), np.int32), "x32": np.empty((rows, 256), np.float32), "xb": np.empty((rows, 256), np.float32)}
        if split:
            out["h128"], out["hb"] = np.empty((rows, 128), np.float32), np.empty((rows, 256), np.float32)
        a = _lib.DebugSgFrontArgs(prec=int(prec), split=int(split), B=b, cap=cap, normalize=int(normalize), f0=f0.ctypes.data, f1=f1.ctypes.data, n0=n0.ctypes.data,
                                  n1=n1.ctypes.data, rows=rows, **{k: v.ctypes.data for k, v in out.items()})
        self._chk(self._l.airfe_debug_sg_front(self._h, C.byref(a)), "airfe_debug_sg_front")
        out["rows_past"], out["Np"], out["M"] = int(a.rows_past), self.np_rows, m
        return out

    def debug_lg_assign(self, md, x32, lens, w, b, prec, form, cap=None, thr=0.1, pad=None):
        """rowdot256 + the assignment tail alone (include/airfe_debug.h, airfe_debug_lg_assign): md, x32 [2B, n, 256], lens [2B] (0 allowed), w [256], b; form 0 the
        similarity matrix + launch_lg_assign, 1 launch_lg_assign_fused.  -> dict z [2B, n], sim, scores [B, n, n], rowlse, collse, rowval, rowarg, colarg [B, n],
        idx [B, cap, 2], score [B, cap], nmatch [B]: the device's buffers as the launches left them, their poison included."""
        f32 = lambda t: np.ascontiguousarray(t, np.float32)
        md, x32, w = f32(md), f32(x32), f32(w)
        lens = np.ascontiguousarray(lens, np.int32).reshape(-1)
        s, n, _ = md.shape
        bb = s // 2
        cap = self.np_rows if cap is None else int(cap)
        out = {"z": np.empty((s, n), np.float32), "sim": np.empty((bb, n, n), np.float32), "scores": np.empty((bb, n, n), np.float32),
               "rowlse": np.empty((bb, n), np.float32), "collse": np.empty((bb, n), np.float32), "rowval": np.empty((bb, n), np.float32),
               "rowarg": np.empty((bb, n), np.int32), "colarg": np.empty((bb, n), np.int32), "idx": np.empty((bb, cap, 2), np.int32),
               "score": np.empty((bb, cap), np.float32), "nmatch": np.empty((bb,), np.int32)}
        assert x32.shape == md.shape and len(lens) == s and s % 2 == 0
        a = _lib.DebugLgAssignArgs(prec=prec, B=bb, n=n, md=md.ctypes.data, x32=x32.ctypes.data, w=w.ctypes.data, b=float(b), lens=lens.ctypes.data, cap=cap,
                                   thr=float(thr), form=int(form), **{k: v.ctypes.data for k, v in out.items()})
        if pad is not None:
            pad = f32(pad)
            a.pad = pad.ctypes.data
        self._chk(self._l.airfe_debug_lg_assign(self._h, C.byref(a)), "airfe_debug_lg_assign")
        return out

    def detector_maps(self, b: int = 1):
        heat = np.empty((b, 512, 512), np.float32)
        nms = np.empty((b, 512, 512), np.float32)
        desc = np.empty((b, 64, 64, 256), np.float32)
        self._chk(self._l.airfe_debug_detector_maps(self._h, b, heat.ctypes.data, nms.ctypes.data, desc.ctypes.data),
                  "airfe_debug_detector_maps")
        return heat, nms, desc

    def debug_detector_tail(self, heat, act, cap, Bs=0, h=512, w=512, sentinel=7.0, want_keep=True):
        """airfe_debug_detector_tail (include/airfe_debug.h): everything the detector runs behind the score head on host score maps heat [B, 512, 512] and convDa
        activations act [B, 64, 64, 256].  Bs = 0: one destination; else images b >= Bs go to the second.  The feature buffers start as `sentinel`, the counts as -1.
        -> dict feat [B, cap, 259] and n [B] (both destinations concatenated in image order), cand_cnt [B], keep [B, 64, 64] uint64 (radius 4 and want_keep; else None),
        nms_map [B, 512, 512] (None where the form wrote none)."""
        heat, act = np.ascontiguousarray(heat, np.float32), np.ascontiguousarray(act, np.float32)
        b = heat.shape[0]
        assert heat.shape == (b, 512, 512) and act.shape == (b, 64, 64, 256)
        b0 = Bs if Bs else b
        feat, n = np.full((b0, cap, FEAT), sentinel, np.float32), np.full((b0,), -1, np.int32)
        feat1, n1 = np.full((b - b0, cap, FEAT), sentinel, np.float32), np.full((b - b0,), -1, np.int32)
        nms = np.full((b, 512, 512), np.nan, np.float32)
        keep = np.zeros((b, 64, 64), np.uint64) if want_keep and self.cfg.nms_radius == 4 else None
        cnt = np.full((b,), -1, np.int32)
        a = _lib.DebugDetectorTailArgs(B=b, Bs=int(Bs), h=int(h), w=int(w), cap=int(cap), heat=heat.ctypes.data, act=act.ctypes.data, feat=feat.ctypes.data, n=n.ctypes.data,
                                       nms_map=nms.ctypes.data, cand_cnt=cnt.ctypes.data)
        if Bs:
            a.feat1, a.n1 = feat1.ctypes.data, n1.ctypes.data
        if keep is not None:
            a.keep = keep.ctypes.data
        self._chk(self._l.airfe_debug_detector_tail(self._h, C.byref(a)), "airfe_debug_detector_tail")
        return {"feat": np.concatenate([feat, feat1]), "n": np.concatenate([n, n1]), "cand_cnt": cnt, "keep": keep, "nms_map": nms if a.nms_map_written else None}

    def debug_line_post(self, la, sc, m2, heat, cap_lines, cap_junctions, nj=None, from_plane=False, h=512, w=512, sentinel=7.0, jmap=None):
        """airfe_debug_line_post (include/airfe_debug.h): the line filter and the junction scan on host stage-1 outputs la [B, ld, 4], sc [B, ld] (m2 [B] lines each) and score
        maps heat [B, 512, 512]; the junction scores come from the dense NMS'd map or (from_plane) from the raw scores under the keep plane.  The output buffers start as
        `sentinel`.  jmap [nj, 512, 512] uint8 (optional) replaces the junction maps the filter wrote before the scan reads them.
        -> dict lines [B, capL, 4] float64, nlines, nfound [B], junc [nj, capJ, 259], njunc, jfound [nj]."""
        la, sc, heat = np.ascontiguousarray(la, np.float32), np.ascontiguousarray(sc, np.float32), np.ascontiguousarray(heat, np.float32)
        m2 = np.ascontiguousarray(m2, np.int32).reshape(-1)
        b, ld = sc.shape
        nj = b if nj is None else int(nj)
        assert la.shape == (b, ld, 4) and heat.shape == (b, 512, 512) and len(m2) == b
        out = {"lines": np.full((b, cap_lines, 4), sentinel, np.float64), "nlines": np.full((b,), -1, np.int32), "nfound": np.full((b,), -1, np.int32),
               "junc": np.full((nj, cap_junctions, FEAT), sentinel, np.float32), "njunc": np.full((nj,), -1, np.int32), "jfound": np.full((nj,), -1, np.int32)}
        a = _lib.DebugLinePostArgs(B=b, nj=nj, ld=ld, h=int(h), w=int(w), capL=int(cap_lines), capJ=int(cap_junctions), from_plane=int(bool(from_plane)), la=la.ctypes.data,
                                   sc=sc.ctypes.data, m2=m2.ctypes.data, heat=heat.ctypes.data, **{k: v.ctypes.data for k, v in out.items()})
        if jmap is not None:
            jmap = np.ascontiguousarray(jmap, np.uint8)
            assert jmap.shape == (nj, 512, 512)
            a.jmap = jmap.ctypes.data
        self._chk(self._l.airfe_debug_line_post(self._h, C.byref(a)), "airfe_debug_line_post")
        return out

    def debug_junction_tail(self, la, sc, m2, heat, act, cap_lines, cap_junctions, nj=None, h=512, w=512, sentinel=7.0):
        """airfe_debug_junction_tail (include/airfe_debug.h): line filter -> junction descriptors as the batched line path runs them, in the form production chooses
        (B > 2 and the context's tuning: the junction list inside the filter and the sampling gather GEMM; else byte maps, scan, dense head, sample_desc), on host stage-1
        outputs la [B, ld, 4], sc [B, ld], m2 [B], score maps heat [B, 512, 512] and convDa activations act [B, 64, 64, 256].  The output buffers start as `sentinel`.
        -> dict lines [B, capL, 4] float64, nlines, nfound [B], junc [nj, capJ, 259], njunc, jfound [nj], fused (bool)."""
        la, sc, heat = np.ascontiguousarray(la, np.float32), np.ascontiguousarray(sc, np.float32), np.ascontiguousarray(heat, np.float32)
        act = np.ascontiguousarray(act, np.float32)
        m2 = np.ascontiguousarray(m2, np.int32).reshape(-1)
        b, ld = sc.shape
        nj = b if nj is None else int(nj)
        assert la.shape == (b, ld, 4) and heat.shape == (b, 512, 512) and act.shape == (b, 64, 64, 256) and len(m2) == b
        out = {"lines": np.full((b, cap_lines, 4), sentinel, np.float64), "nlines": np.full((b,), -1, np.int32), "nfound": np.full((b,), -1, np.int32),
               "junc": np.full((nj, cap_junctions, FEAT), sentinel, np.float32), "njunc": np.full((nj,), -1, np.int32), "jfound": np.full((nj,), -1, np.int32)}
        a = _lib.DebugJunctionTailArgs(B=b, nj=nj, ld=ld, h=int(h), w=int(w), capL=int(cap_lines), capJ=int(cap_junctions), la=la.ctypes.data, sc=sc.ctypes.data,
                                       m2=m2.ctypes.data, heat=heat.ctypes.data, act=act.ctypes.data, **{k: v.ctypes.data for k, v in out.items()})
        self._chk(self._l.airfe_debug_junction_tail(self._h, C.byref(a)), "airfe_debug_junction_tail")
        out["fused"] = bool(a.fused)
        return out

    def debug_line_mid(self, juncs_pred, lines_pred, thin, aux, loi, iskeep=None, idx_min=None, idx_max=None, j2l=0, s1_form=2, wgs=0):
        """airfe_debug_line_mid (include/airfe_debug.h): the junction-to-line match, the kept list and unique pairs, the junction projections and stage 1 on host tensors
        juncs_pred [B, 300, 2], lines_pred [B, 49152, 4], thin / aux [B, 4, 128, 128], loi [B, 16384, 128] (pixel-major), iskeep / idx_min / idx_max [B, 49152] (j2l = 0).
        -> dict of whole device buffers, 0xFF bytes where the run wrote nothing: iskeep, idx_min, idx_max [B, 49152], counts [B, 2], keep [B, 49152], pairs [B, 45056, 2],
        rep [B, 45056], head4, prop4, lines_adjusted [B, 45056, 4], scores_line [B, 45056], ridx [B, 300, 4], proj [B, 300, 256], table_dirty [B]."""
        f = lambda x: np.ascontiguousarray(x, np.float32)
        juncs_pred, lines_pred, thin, aux, loi = f(juncs_pred), f(lines_pred), f(thin), f(aux), f(loi)
        b, n, cap = juncs_pred.shape[0], 3 * 128 * 128, 45056
        assert juncs_pred.shape == (b, 300, 2) and lines_pred.shape == (b, n, 4) and thin.shape == aux.shape == (b, 4, 128, 128) and loi.shape == (b, 128 * 128, 128)
        poison = lambda shape, dt: np.full(shape, -1, np.int32).view(dt) if dt == np.float32 else np.full(shape, -1, np.int32)
        out = {"iskeep": poison((b, n), np.float32), "idx_min": poison((b, n), np.float32), "idx_max": poison((b, n), np.float32), "counts": poison((b, 2), np.int32),
               "keep": poison((b, n), np.int32), "pairs": poison((b, cap, 2), np.int32), "rep": poison((b, cap), np.int32), "head4": poison((b, cap, 4), np.float32),
               "prop4": poison((b, cap, 4), np.float32), "ridx": poison((b, 300, 4), np.int32), "proj": poison((b, 300, 256), np.float32),
               "lines_adjusted": poison((b, cap, 4), np.float32), "scores_line": poison((b, cap), np.float32), "table_dirty": poison((b,), np.int32)}
        a = _lib.DebugLineMidArgs(B=b, j2l=int(j2l), s1_form=int(s1_form), wgs=int(wgs), juncs_pred=juncs_pred.ctypes.data, lines_pred=lines_pred.ctypes.data,
                                  thin=thin.ctypes.data, aux=aux.ctypes.data, loi=loi.ctypes.data, **{k: v.ctypes.data for k, v in out.items()})
        ins = [None if x is None else f(x) for x in (iskeep, idx_min, idx_max)]
        for name, x in zip(("iskeep_in", "idx_min_in", "idx_max_in"), ins):
            if x is not None:
                assert x.shape == (b, n)
                setattr(a, name, x.ctypes.data)
        self._chk(self._l.airfe_debug_line_mid(self._h, C.byref(a)), "airfe_debug_line_mid")
        return out

    # stage-block offsets in floats (csrc/airfe_host.h, SG_*): juncs_pred | lines_pred | iskeep | idx_min | idx_max | thin | aux, the stride rounded up to 64
    S0_STAGE = {"lines_pred": (600, 3 * 16384 * 4), "thin": (600 + 7 * 3 * 16384, 4 * 16384), "aux": (600 + 7 * 3 * 16384 + 4 * 16384, 4 * 16384)}
    S0_STAGE_FLOATS = (600 + 7 * 3 * 16384 + 8 * 16384 + 63) // 64 * 64

    def debug_s0_decode(self, rows=None, ld=160, off=128, ta8=True, loi=False, jnms=True, x=None, w=None, b=None, prec=1, wgs=0, two_pass=False):
        """airfe_debug_s0_decode (include/airfe_debug.h): the stage-0 decode alone.  rows [B, 16384, ld] fp32 head rows (the 17 decoded channels from column off) through
        launch_s0_decode; or x [B * 16384, 128] line features with a head w [17, 128], b [17] in the 2-byte type prec through launch_s0_head_decode(wgs), with two_pass
        through launch_gemm + launch_s0_decode(32, 0).
        -> dict of whole device buffers, 0xFF bytes where the run wrote nothing: stage [B, S0_STAGE_FLOATS] with its views lines_pred [B, 49152, 4] and thin / aux
        [B, 4, 128, 128]; jloc, jnms [B, 128, 128]; joff [B, 2, 128, 128]; ta8 [B, 16384, 8]; loi [128, 128, 128] (CHW, image 0); head_rows [B, 16384, 32] (two_pass)."""
        f = lambda t: np.ascontiguousarray(t, np.float32)
        npx, sf = 128 * 128, self.S0_STAGE_FLOATS
        a = _lib.DebugS0DecodeArgs(want_ta8=int(bool(ta8)), want_loi=int(bool(loi)), want_jnms=int(bool(jnms)), prec=int(prec), wgs=int(wgs), stage_floats=sf)
        if rows is not None:
            assert x is None and not two_pass
            rows = f(rows)
            bb = rows.shape[0]
            assert rows.shape == (bb, npx, ld)
            a.mode, a.ld, a.off, a.rows = 0, int(ld), int(off), rows.ctypes.data
        else:
            x, w, b = f(x), f(w), f(b)
            bb = x.shape[0] // npx
            assert x.shape == (bb * npx, 128) and w.shape == (17, 128) and b.shape == (17,)
            a.mode, a.x, a.w, a.b = (2 if two_pass else 1), x.ctypes.data, w.ctypes.data, b.ctypes.data
        poison = lambda *shape: np.full(shape, -1, np.int32).view(np.float32)
        out = {"stage": poison(bb, sf), "jloc": poison(bb, 128, 128), "joff": poison(bb, 2, 128, 128), "jnms": poison(bb, 128, 128), "ta8": poison(bb, npx, 8),
               "loi": poison(128, 128, 128)}
        if two_pass:
            out["head_rows"] = poison(bb, npx, 32)
        a.B = bb
        for k, v in out.items():
            setattr(a, k, v.ctypes.data)
        self._chk(self._l.airfe_debug_s0_decode(self._h, C.byref(a)), "airfe_debug_s0_decode")
        for k, (o, n) in self.S0_STAGE.items():
            v = out["stage"][:, o:o + n]
            out[k] = v.reshape(bb, 3 * npx, 4) if k == "lines_pred" else v.reshape(bb, 4, 128, 128)
        return out

    def debug_junctions_topk(self, jloc, joff):
        """airfe_debug_junctions_topk (include/airfe_debug.h): jloc [B, 128, 128], joff [B, 2, 128, 128] -> juncs_pred [B, 300, 2]"""
        jloc, joff = np.ascontiguousarray(jloc, np.float32), np.ascontiguousarray(joff, np.float32)
        b = jloc.shape[0]
        assert jloc.shape == (b, 128, 128) and joff.shape == (b, 2, 128, 128)
        out = np.full((b, 300, 2), np.nan, np.float32)
        self._chk(self._l.airfe_debug_junctions_topk(self._h, jloc.ctypes.data, joff.ctypes.data, b, out.ctypes.data), "airfe_debug_junctions_topk")
        return out

    def debug_preprocess(self, gray):
        gray = np.ascontiguousarray(gray, np.uint8)
        out = np.empty((512, 512), np.float32)
        self._chk(self._l.airfe_debug_preprocess(self._h, gray.ctypes.data, gray.shape[0], gray.shape[1], gray.strides[0],
                                                 out.ctypes.data), "airfe_debug_preprocess")
        return out

    def debug_conv3x3(self, x, w, b, pool=False):
        x = np.ascontiguousarray(x, np.float32); w = np.ascontiguousarray(w, np.float32); b = np.ascontiguousarray(b, np.float32)
        bb, cin, hh, ww = x.shape
        cout = w.shape[0]
        ho, wo = (hh // 2, ww // 2) if pool else (hh, ww)
        y = np.empty((bb, cout, ho, wo), np.float32)
        self._chk(self._l.airfe_debug_conv3x3(self._h, x.ctypes.data, bb, cin, hh, ww, w.ctypes.data, b.ctypes.data, cout,
                                              int(pool), y.ctypes.data), "airfe_debug_conv3x3")
        return y

    def debug_conv(self, w, b, prec, x=None, img=None, w1a=None, b1a=None, pool=False, out_pad=1, relu=True, wgs=256):
        """airfe_debug_conv (include/airfe_debug.h): one 3x3 convolution launch on host tensors, x [B, cin, H, W] (plain form) or img [B, H, W] with w1a [64, 9] and
        b1a [64] (fused conv1a -> conv1b).  prec names the context's 2-byte type (the words are converted with it).  Returns dict: raw = the device buffer's words
        [B, Ho + 2 p, Wo + 2 p, cout] (uint16), guard_lo / guard_hi = the words before and behind it, y = its interior as float32 [B, cout, Ho, Wo]."""
        f32 = lambda t: None if t is None else np.ascontiguousarray(t, np.float32)
        x, img, w1a, b1a, w, b = map(f32, (x, img, w1a, b1a, w, b))
        src = x if x is not None else img
        bb, hh, ww = src.shape[0], src.shape[-2], src.shape[-1]
        cout, cin = w.shape[0], w.shape[1]
        p = int(out_pad)
        ho, wo = (hh // 2, ww // 2) if pool else (hh, ww)
        guard = (wo + 2 * p) * cout
        words = bb * (ho + 2 * p) * guard
        raw = np.zeros(words + 2 * guard, np.uint16)
        ptr = lambda t: None if t is None else t.ctypes.data
        a = _lib.DebugConvArgs(x=ptr(x), img=ptr(img), w1a=ptr(w1a), b1a=ptr(b1a), w=ptr(w), b=ptr(b), cin=cin, cout=cout, B=bb, H=hh, W=ww, pool=int(pool), out_pad=p,
                               relu=int(relu), wgs=int(wgs), y_words=raw.size, y_raw=ptr(raw))
        self._chk(self._l.airfe_debug_conv(self._h, C.byref(a)), "airfe_debug_conv")
        buf = raw[guard:guard + words].reshape(bb, ho + 2 * p, wo + 2 * p, cout)
        inner = np.ascontiguousarray(buf[:, p:p + ho, p:p + wo, :])
        y = inner.view(np.float16).astype(np.float32) if prec == 1 else (inner.astype(np.uint32) << 16).view(np.float32)
        return {"raw": buf, "guard_lo": raw[:guard], "guard_hi": raw[guard + words:], "y": np.ascontiguousarray(y.transpose(0, 3, 1, 2))}

    def debug_gemm(self, x, w, b, relu=False):
        x = np.ascontiguousarray(x, np.float32); w = np.ascontiguousarray(w, np.float32); b = np.ascontiguousarray(b, np.float32)
        m, k = x.shape
        n = w.shape[0]
        y = np.empty((m, n), np.float32)
        self._chk(self._l.airfe_debug_gemm(self._h, x.ctypes.data, m, k, w.ctypes.data, b.ctypes.data, n, int(relu),
                                           y.ctypes.data), "airfe_debug_gemm")
        return y

    # kernel names of airfe_debug_linear's `kernel` (include/airfe_debug.h)
    DEBUG_KERNELS = {"dispatch": 0, "small": 1, "tiled": 2, "gemm8": 3, "gemmr": 4, "gemmr_gather": 5, "gemmr_gather128": 6}

    def debug_linear(self, x1, w, b, prec, epi=0, act=0, x2=None, rowidx=None, rot=None, Np=0, x32=None, d2s=None, kernel="dispatch", gr_wgs=0):
        """One form of the GEMM family (include/airfe_debug.h, airfe_debug_linear) on host fp32 tensors: x1 [M, K1] ([src_rows, K1] with rowidx [M]),
        x2 [M, K - K1], w [N, K], b [N]; rot = (cos, sin) [M, 32]; x32 [M, N] (EPI_RESID); d2s = (hc, wc) (EPI_SOFTMAX_D2S).  Returns out in the
        kernel's own layout, and for EPI_HEADS with N = 512 (q, k), for EPI_RESID (xb, x32), for EPI_SOFTMAX_D2S (heat, flag)."""
        f32 = lambda t: None if t is None else np.ascontiguousarray(t, np.float32)
        x1, w, b, x2, x32 = f32(x1), f32(w), f32(b), f32(x2), (None if x32 is None else np.array(x32, np.float32, copy=True))
        n, k = w.shape
        m = len(rowidx) if rowidx is not None else x1.shape[0]
        a = _lib.DebugLinearArgs(prec=prec, M=m, K=k, K1=x1.shape[1], N=n, x1=x1.ctypes.data, w=w.ctypes.data, b=b.ctypes.data, epi=epi, act=act, Np=Np, H=4,
                                 kernel=self.DEBUG_KERNELS[kernel], gr_wgs=gr_wgs)
        keep = []
        if x2 is not None:
            a.x2 = x2.ctypes.data
        if rowidx is not None:
            ri = np.ascontiguousarray(rowidx, np.int32)
            keep.append(ri)
            a.rowidx, a.src_rows = ri.ctypes.data, x1.shape[0]
        if rot is not None:
            rc, rs = f32(rot[0]), f32(rot[1])
            keep += [rc, rs]
            a.rot_cos, a.rot_sin = rc.ctypes.data, rs.ctypes.data
        if x32 is not None:
            a.x32 = x32.ctypes.data
        flag = np.zeros(1, np.int32)
        out2 = None
        if epi == 5:
            hc, wc = d2s
            a.d2s_hc, a.d2s_wc, a.flag = hc, wc, flag.ctypes.data
            out = np.empty((m // (hc * wc), 8 * hc, 8 * wc), np.float32)
        elif epi in (3, 4):
            s = m // Np
            out = np.empty((s, 4, Np, 64) if epi == 3 else (s, 4, 64, Np), np.float32)
            if epi == 3 and n == 512:
                out2 = np.empty_like(out)
                a.out2 = out2.ctypes.data
        else:
            out = np.empty((m, n), np.float32)
        a.out = out.ctypes.data
        self._chk(self._l.airfe_debug_linear(self._h, C.byref(a)), "airfe_debug_linear")
        if epi == 5:
            return out, int(flag[0])
        if epi == 2:
            return out, x32
        return (out, out2) if out2 is not None else out

    def debug_qkv(self, x, wqk, bqk, wv, bv, prec, Np, rot=None, pair=True, gr_wgs=0):
        """airfe_debug_qkv: x [M, 256] -> (q, k or None, vt): q / k [S, 4, Np, 64], vt [S, 4, 64, Np]; pair: one gemmr_pair launch"""
        f32 = lambda t: np.ascontiguousarray(t, np.float32)
        x, wqk, bqk, wv, bv = f32(x), f32(wqk), f32(bqk), f32(wv), f32(bv)
        m, nqk, s = x.shape[0], wqk.shape[0], x.shape[0] // Np
        q = np.empty((s, 4, Np, 64), np.float32)
        k = np.empty_like(q) if nqk == 512 else None
        vt = np.empty((s, 4, 64, Np), np.float32)
        rc, rs = (f32(rot[0]), f32(rot[1])) if rot is not None else (None, None)
        ptr = lambda t: None if t is None else t.ctypes.data
        self._chk(self._l.airfe_debug_qkv(self._h, prec, m, Np, ptr(x), ptr(wqk), ptr(bqk), nqk, ptr(wv), ptr(bv), ptr(rc), ptr(rs), int(pair), gr_wgs, ptr(q),
                                          ptr(k), ptr(vt)), "airfe_debug_qkv")
        return q, k, vt

    def debug_lg_block(self, attn, x32, w1, b1, w2, b2, prec, gamma=None, beta=None, wo=None, bo=None, relu=False, tokens_per_wg=128, mixed=False,
                       nqk=None, nv=None, rot=None, Np=0):
        """airfe_debug_lg_block: the fused post-attention block on host tensors.  nqk = (w [n, 256], b), nv = (w [256, 256], b): the next layer's
        projections.  Returns dict x32, xb, q, k, vt (None where absent) and rows_past (rows past M written in x32, xb, q, k, vt)."""
        f32 = lambda t: None if t is None else np.ascontiguousarray(t, np.float32)
        m = attn.shape[0]
        attn, w1, b1, w2, b2, gamma, beta, wo, bo = map(f32, (attn, w1, b1, w2, b2, gamma, beta, wo, bo))
        x32 = np.array(x32, np.float32, copy=True)
        xb = np.empty_like(x32)
        ptr = lambda t: None if t is None else t.ctypes.data
        a = _lib.DebugLgBlockArgs(prec=prec, M=m, attn=ptr(attn), x32=ptr(x32), xb=ptr(xb), wo=ptr(wo), bo=ptr(bo), w1=ptr(w1), b1=ptr(b1), gamma=ptr(gamma),
                                  beta=ptr(beta), w2=ptr(w2), b2=ptr(b2), relu=int(relu), tokens_per_wg=tokens_per_wg, mixed=int(mixed), Np=Np)
        q = k = vt = None
        keep = []
        if nqk is not None:
            (qw, qb), (vw, vb) = map(lambda p: (f32(p[0]), f32(p[1])), (nqk, nv))
            keep += [qw, qb, vw, vb]
            s = m // Np
            q, vt = np.empty((s, 4, Np, 64), np.float32), np.empty((s, 4, 64, Np), np.float32)
            a.nqk_n, a.nqk_w, a.nqk_b, a.nv_w, a.nv_b, a.q, a.vt = qw.shape[0], ptr(qw), ptr(qb), ptr(vw), ptr(vb), ptr(q), ptr(vt)
            if qw.shape[0] == 512:
                k = np.empty_like(q)
                a.k = ptr(k)
        if rot is not None:
            rc, rs = f32(rot[0]), f32(rot[1])
            keep += [rc, rs]
            a.rot_cos, a.rot_sin = ptr(rc), ptr(rs)
        self._chk(self._l.airfe_debug_lg_block(self._h, C.byref(a)), "airfe_debug_lg_block")
        return {"x32": x32, "xb": xb, "q": q, "k": k, "vt": vt, "rows_past": list(a.rows_past)}

    def debug_ln_gelu(self, h, gamma, beta, prec):
        """airfe_debug_ln_gelu: launch_ln_gelu in place on h [M, 512] (rounded to the 2-byte type on the way in) -> the kernel's result"""
        h = np.array(h, np.float32, copy=True)
        gamma, beta = np.ascontiguousarray(gamma, np.float32), np.ascontiguousarray(beta, np.float32)
        self._chk(self._l.airfe_debug_ln_gelu(self._h, prec, h.ctypes.data, gamma.ctypes.data, beta.ctypes.data, h.shape[0]), "airfe_debug_ln_gelu")
        return h

    def debug_attention(self, q, k, v, lens, cross=False, prec=None, raw=False):
        """The matcher's flash attention alone (include/airfe_debug.h): q, k, v [S, H, n, 64] fp32 (scale and log2 e already inside q / k), lens [S] -> out [S, n, H * 64].
        prec None: airfe_debug_attention (the context's matcher_precision, an output buffer as the allocator left it).  prec 0 (bf16) / 1 (fp16):
        airfe_debug_attention_args with the canary — rows that the launch did not write come back NaN; raw: -> (out [S, Np, H * 64] with every padded row, rows_past)."""
        q = np.ascontiguousarray(q, np.float32); k = np.ascontiguousarray(k, np.float32); v = np.ascontiguousarray(v, np.float32)
        lens = np.ascontiguousarray(lens, np.int32)
        s, h, n, d = q.shape
        assert d == 64 and k.shape == q.shape and v.shape == q.shape and lens.shape == (s,)
        if prec is None:
            assert not raw, "raw rows come from airfe_debug_attention_args: give prec"
            out = np.empty((s, n, h * 64), np.float32)
            self._chk(self._l.airfe_debug_attention(self._h, q.ctypes.data, k.ctypes.data, v.ctypes.data, lens.ctypes.data, s, h, n, int(cross), out.ctypes.data),
                      "airfe_debug_attention")
            return out
        out = np.empty((s, (n + 15) // 16 * 16 if raw else n, h * 64), np.float32)
        a = _lib.DebugAttentionArgs(prec=int(prec), S=s, H=h, n=n, cross=int(cross), q=q.ctypes.data, k=k.ctypes.data, v=v.ctypes.data, lens=lens.ctypes.data,
                                    canary=1, raw=int(raw), out=out.ctypes.data)
        self._chk(self._l.airfe_debug_attention_args(self._h, C.byref(a)), "airfe_debug_attention_args")
        return (out, a.rows_past) if raw else out

    # ---------------------------------------------------------------- device-resident batch (torch plumbing)
    def detect_batch_dev(self, gray_t, feat_t, n_t, stream=None):
        b, h, w = gray_t.shape
        self._chk(self._l.airfe_detect_points_batch_dev(self._h, gray_t.data_ptr(), b, h, w, gray_t.stride(1),
                                                        gray_t.stride(0), feat_t.data_ptr(), feat_t.shape[1],
                                                        n_t.data_ptr(), self._stream(stream)), "airfe_detect_points_batch_dev")

    def fundamental_ransac(self, f0: np.ndarray, f1: np.ndarray, idx: np.ndarray, score: np.ndarray):
        """F-matrix RANSAC on ONE match list (airfe_fundamental_ransac ≙ point_matcher.cc:95-104; contract: include/airfe.h): f0 [n0,259], f1 [n1,259]
        rows in original pixels, idx [m,2] (index into f0, into f1), score [m] -> (idx [k,2], score [k]): the kept matches in their order."""
        f0 = np.ascontiguousarray(f0, dtype=np.float32).reshape(-1, FEAT)
        f1 = np.ascontiguousarray(f1, dtype=np.float32).reshape(-1, FEAT)
        idx = np.array(idx, dtype=np.int32, copy=True).reshape(-1, 2)
        score = np.array(score, dtype=np.float32, copy=True).reshape(-1)
        if len(score) != len(idx):
            raise AirfeError("fundamental_ransac: idx and score differ in length")
        k = C.c_int(0)
        self._chk(self._l.airfe_fundamental_ransac(self._h, f0.ctypes.data, len(f0), f1.ctypes.data, len(f1), idx.ctypes.data, score.ctypes.data, len(idx),
                                                   C.byref(k)), "airfe_fundamental_ransac")
        return idx[:k.value], score[:k.value]

    def fundamental_ransac_batch_dev(self, f0_t, f1_t, idx_t, score_t, nm_t, F_t=None, stream=None):
        """airfe_fundamental_ransac_batch_dev: f0_t / f1_t [B,cap,259], idx_t [B,mcap,2], score_t [B,mcap], nm_t [B] (filtered in place), F_t [B,9] float64."""
        self._chk(self._l.airfe_fundamental_ransac_batch_dev(self._h, f0_t.data_ptr(), None, f1_t.data_ptr(), None, f0_t.shape[0], f0_t.shape[1],
                                                             idx_t.data_ptr(), score_t.data_ptr(), idx_t.shape[1], nm_t.data_ptr(),
                                                             None if F_t is None else F_t.data_ptr(), self._stream(stream)),
                  "airfe_fundamental_ransac_batch_dev")

    def pnp_ransac(self, obj: np.ndarray, img: np.ndarray, K):
        """PnP RANSAC on ONE problem (airfe_pnp_ransac ≙ cv::solvePnPRansac in SolvePnPWithCV, g2o_optimization.cc:1085-1134; contract: include/airfe.h):
        obj [n,3], img [n,2] (doubles; rounded to float as cv::Point3f / Point2f), K = (fx, fy, cx, cy) -> dict(Twc [4,4], Rt [12] (Rcw row-major, tcw),
        inlier [n] uint8, count)."""
        obj = np.ascontiguousarray(obj, np.float64).reshape(-1, 3)
        img = np.ascontiguousarray(img, np.float64).reshape(-1, 2)
        if len(obj) != len(img):
            raise AirfeError("pnp_ransac: obj and img differ in length")
        k = np.ascontiguousarray(K, np.float64).reshape(4)
        Twc, Rt = np.zeros(16), np.zeros(12)
        mask = np.zeros(max(len(obj), 1), np.uint8)
        cnt = C.c_int(0)
        self._chk(self._l.airfe_pnp_ransac(self._h, obj.ctypes.data, img.ctypes.data, len(obj), k.ctypes.data, Twc.ctypes.data, Rt.ctypes.data,
                                           mask.ctypes.data, C.byref(cnt)), "airfe_pnp_ransac")
        return dict(Twc=Twc.reshape(4, 4), Rt=Rt, inlier=mask[:len(obj)], count=cnt.value)

    def pnp_ransac_batch_dev(self, obj_t, img_t, n_t, K, Twc_t, inlier_t, count_t, Rt_t=None, stream=None):
        """airfe_pnp_ransac_batch_dev: obj_t [B,ncap,3] / img_t [B,ncap,2] float32, n_t [B] int32 -> Twc_t [B,16] float64, inlier_t [B,ncap] uint8,
        count_t [B] int32, Rt_t [B,12] float64 (optional)."""
        k = np.ascontiguousarray(K, np.float64).reshape(4)
        self._chk(self._l.airfe_pnp_ransac_batch_dev(self._h, obj_t.data_ptr(), img_t.data_ptr(), n_t.data_ptr(), obj_t.shape[0], obj_t.shape[1],
                                                     k.ctypes.data, Twc_t.data_ptr(), None if Rt_t is None else Rt_t.data_ptr(), inlier_t.data_ptr(),
                                                     count_t.data_ptr(), self._stream(stream)), "airfe_pnp_ransac_batch_dev")

    def stereo_points(self, cam, featL: np.ndarray, featR: np.ndarray, idx: np.ndarray):
        """Frame::AddRightFeatures + BackProjectPoint on ONE stereo list (airfe_stereo_points): cam = (min_x_diff, max_x_diff, max_y_diff, bf, fx, fy, cx, cy),
        featL [nL,259], featR [nR,259], idx [m,2] (left, right) -> dict(u_right [nL], depth [nL] (-1 unset), xyz [nL,3] (NaN unset), good)."""
        cam = np.ascontiguousarray(cam, np.float64).reshape(8)
        featL = np.ascontiguousarray(featL, np.float32).reshape(-1, FEAT)
        featR = np.ascontiguousarray(featR, np.float32).reshape(-1, FEAT)
        idx = np.ascontiguousarray(idx, np.int32).reshape(-1, 2)
        nL = len(featL)
        u, d, xyz = np.empty(max(nL, 1)), np.empty(max(nL, 1)), np.empty((max(nL, 1), 3))
        good = C.c_int(0)
        self._chk(self._l.airfe_stereo_points(self._h, cam.ctypes.data, featL.ctypes.data, nL, featR.ctypes.data, len(featR), idx.ctypes.data, len(idx),
                                              u.ctypes.data, d.ctypes.data, xyz.ctypes.data, C.byref(good)), "airfe_stereo_points")
        return dict(u_right=u[:nL], depth=d[:nL], xyz=xyz[:nL], good=good.value)

    def stereo_points_batch_dev(self, cam, featL_t, nL_t, featR_t, nR_t, idx_t, nm_t, u_right_t, depth_t, xyz_t, good_t, stream=None):
        """airfe_stereo_points_batch_dev: feat [B,cap,259], n [B], idx_t [B,mcap,2], nm_t [B] -> u_right_t / depth_t [B,cap], xyz_t [B,cap,3] float64,
        good_t [B] int32."""
        cam = np.ascontiguousarray(cam, np.float64).reshape(8)
        self._chk(self._l.airfe_stereo_points_batch_dev(self._h, cam.ctypes.data, featL_t.data_ptr(), nL_t.data_ptr(), featR_t.data_ptr(), nR_t.data_ptr(),
                                                        featL_t.shape[0], featL_t.shape[1], idx_t.data_ptr(), nm_t.data_ptr(), idx_t.shape[1],
                                                        u_right_t.data_ptr(), depth_t.data_ptr(), xyz_t.data_ptr(), good_t.data_ptr(), self._stream(stream)),
                  "airfe_stereo_points_batch_dev")

    def stereo_lines(self, cam, lines_left: np.ndarray, lines_right: np.ndarray, line_matches: np.ndarray, Twc=None):
        """The loop of Frame::AddRightFeatures over the line matches (src/frame.cc:185-191) + TriangulateByStereo + ComputeLine3DFromEndpoints on ONE
        frame (airfe_stereo_lines, host only): cam as stereo_points, lines [n,4] float64, line_matches [nL] (match_lines' output), Twc [4,4] or None
        -> dict(lines_right_sel [nL,4], right_valid [nL] uint8, status [nL] int32, endpoints [nL,6], plucker [nL,6] (NaN unset), count [3] int32)."""
        cam = np.ascontiguousarray(cam, np.float64).reshape(8)
        ll = np.ascontiguousarray(lines_left, np.float64).reshape(-1, 4)
        lr = np.ascontiguousarray(lines_right, np.float64).reshape(-1, 4)
        lm = np.ascontiguousarray(line_matches, np.int32).reshape(-1)
        if len(lm) != len(ll):
            raise ValueError("stereo_lines: one match per left line")
        twc = None if Twc is None else np.ascontiguousarray(Twc, np.float64).reshape(16)
        n = len(ll)
        m = max(n, 1)
        sel, valid, status = np.empty((m, 4)), np.empty(m, np.uint8), np.empty(m, np.int32)
        ends, plk, count = np.empty((m, 6)), np.empty((m, 6)), np.empty(3, np.int32)
        self._chk(self._l.airfe_stereo_lines(self._h, cam.ctypes.data, ll.ctypes.data, n, lr.ctypes.data if len(lr) else None, len(lr), lm.ctypes.data,
                                             None if twc is None else twc.ctypes.data, sel.ctypes.data, valid.ctypes.data, status.ctypes.data,
                                             ends.ctypes.data, plk.ctypes.data, count.ctypes.data), "airfe_stereo_lines")
        return dict(lines_right_sel=sel[:n], right_valid=valid[:n], status=status[:n], endpoints=ends[:n], plucker=plk[:n], count=count)

    def stereo_lines_batch_dev(self, cam, lines_left_t, nlines_left_t, lines_right_t, nlines_right_t, line_matches_t, Twc_t, lines_right_sel_t,
                               right_valid_t, status_t, endpoints_t, plucker_t, count_t, stream=None):
        """airfe_stereo_lines_batch_dev: lines [B,capL,4] float64 + nlines [B] per side (the halves of stereo_plnet_batch_dev's line buffer, in place),
        line_matches_t [B,capL] int32, Twc_t [B,16] float64 or None -> lines_right_sel_t [B,capL,4], right_valid_t [B,capL] uint8, status_t [B,capL]
        int32, endpoints_t / plucker_t [B,capL,6] float64, count_t [B,3] int32."""
        cam = np.ascontiguousarray(cam, np.float64).reshape(8)
        self._chk(self._l.airfe_stereo_lines_batch_dev(
            self._h, cam.ctypes.data, lines_left_t.data_ptr(), nlines_left_t.data_ptr(), lines_right_t.data_ptr(), nlines_right_t.data_ptr(),
            lines_left_t.shape[1], line_matches_t.data_ptr(), None if Twc_t is None else Twc_t.data_ptr(), lines_left_t.shape[0],
            lines_right_sel_t.data_ptr(), right_valid_t.data_ptr(), status_t.data_ptr(), endpoints_t.data_ptr(), plucker_t.data_ptr(), count_t.data_ptr(),
            self._stream(stream)), "airfe_stereo_lines_batch_dev")

    def stereo_line_landmarks_batch_dev(self, cam, lines_left_t, nlines_left_t, lines_right_t, nlines_right_t, featL_t, nL_t, featR_t, nR_t, idx_t, nm_t,
                                        Twc_t, relL, relR, line_matches_t, lines_right_sel_t, right_valid_t, status_t, endpoints_t, plucker_t, count_t,
                                        stream=None):
        """airfe_stereo_line_landmarks_batch_dev: the line half of a stereo keyframe on one stream (assign_points_to_lines_batch_dev on both sides,
        match_lines_batch_dev with the band cam[0:3], stereo_lines_batch_dev).  relL / relR = (row_ptr [B,capL+1] i32, pt_idx [B,capE] i32, pt_dist
        [B,capE] f64, total [B] i32 or None): the caller's relation buffers; line_matches_t [B,capL] i32; the rest as stereo_lines_batch_dev."""
        cam = np.ascontiguousarray(cam, np.float64).reshape(8)
        tot = [None if r[3] is None else r[3].data_ptr() for r in (relL, relR)]
        self._chk(self._l.airfe_stereo_line_landmarks_batch_dev(
            self._h, cam.ctypes.data, lines_left_t.data_ptr(), nlines_left_t.data_ptr(), lines_right_t.data_ptr(), nlines_right_t.data_ptr(),
            lines_left_t.shape[1], featL_t.data_ptr(), nL_t.data_ptr(), featR_t.data_ptr(), nR_t.data_ptr(), featL_t.shape[1], idx_t.data_ptr(),
            nm_t.data_ptr(), idx_t.shape[1], None if Twc_t is None else Twc_t.data_ptr(), lines_left_t.shape[0], relL[0].data_ptr(), relL[1].data_ptr(),
            relL[2].data_ptr(), tot[0], relR[0].data_ptr(), relR[1].data_ptr(), relR[2].data_ptr(), tot[1], relL[1].shape[1],
            line_matches_t.data_ptr(), lines_right_sel_t.data_ptr(), right_valid_t.data_ptr(), status_t.data_ptr(), endpoints_t.data_ptr(),
            plucker_t.data_ptr(), count_t.data_ptr(), self._stream(stream)), "airfe_stereo_line_landmarks_batch_dev")

    def track_pose_batch_dev(self, K, xyz_t, feat_t, tidx_t, ntrack_t, Twc_t, mask_t, count_t, Rt_t=None, stream=None):
        """airfe_track_pose_batch_dev: keyframe points xyz_t [B,capK,3] float64, current rows feat_t [B,cap,259], temporal lists tidx_t [B,mcap,2]
        (keyframe, current) + ntrack_t [B] -> Twc_t [B,16], mask_t [B,mcap] uint8 (per list entry), count_t [B], Rt_t [B,12] (optional)."""
        k = np.ascontiguousarray(K, np.float64).reshape(4)
        self._chk(self._l.airfe_track_pose_batch_dev(self._h, k.ctypes.data, xyz_t.data_ptr(), xyz_t.shape[1], feat_t.data_ptr(), feat_t.shape[1],
                                                     tidx_t.data_ptr(), ntrack_t.data_ptr(), tidx_t.shape[1], tidx_t.shape[0], Twc_t.data_ptr(),
                                                     None if Rt_t is None else Rt_t.data_ptr(), mask_t.data_ptr(), count_t.data_ptr(),
                                                     self._stream(stream)), "airfe_track_pose_batch_dev")

    @staticmethod
    def _tcb(Tcb):
        """(keep-alive array, pointer or None) of Tcb = (Rcb row-major, tcb) [12], a 4x4 Tcb, or None (identity)"""
        if Tcb is None:
            return None, None
        t = np.ascontiguousarray(Tcb, np.float64)
        if t.size == 16:
            t = np.ascontiguousarray(np.concatenate([t.reshape(4, 4)[:3, :3].reshape(9), t.reshape(4, 4)[:3, 3]]))
        t = t.reshape(12)
        return t, t.ctypes.data

    def frame_optimize(self, X: np.ndarray, obs: np.ndarray, cam, thr, Twc0, Tcb=None):
        """Pose-only frame optimisation on ONE problem (airfe_frame_optimize ≙ the vision-only, points-only FrameOptimization of tracking,
        g2o_optimization.cc:446-898; contract: include/airfe.h "Frame optimisation"): X [n,3] map points, obs [n,3] = (x, y, u_right; stereo iff
        u_right > 0), cam = (fx, fy, cx, cy, bf), thr = (mono, stereo) chi-square thresholds, Twc0 [4,4] the start pose, Tcb (optional)
        -> dict(Twc [4,4], Rt [12] (Rcw row-major, tcw), inlier [n] uint8, num_inliers)."""
        X = np.ascontiguousarray(X, np.float64).reshape(-1, 3)
        obs = np.ascontiguousarray(obs, np.float64).reshape(-1, 3)
        if len(X) != len(obs):
            raise AirfeError("frame_optimize: X and obs differ in length")
        cam = np.ascontiguousarray(cam, np.float64).reshape(5)
        thr = np.ascontiguousarray(thr, np.float64).reshape(2)
        T0 = np.ascontiguousarray(Twc0, np.float64).reshape(16)
        keep, tcb = self._tcb(Tcb)
        Twc, Rt = np.zeros(16), np.zeros(12)
        mask = np.zeros(max(len(X), 1), np.uint8)
        num = C.c_int(0)
        self._chk(self._l.airfe_frame_optimize(self._h, X.ctypes.data, obs.ctypes.data, len(X), cam.ctypes.data, tcb, thr.ctypes.data, T0.ctypes.data,
                                               Twc.ctypes.data, Rt.ctypes.data, mask.ctypes.data, C.byref(num)), "airfe_frame_optimize")
        return dict(Twc=Twc.reshape(4, 4), Rt=Rt, inlier=mask[:len(X)], num_inliers=num.value)

    def frame_optimize_batch_dev(self, X_t, obs_t, n_t, Twc0_t, cam, thr, Twc_t, inlier_t, num_t, Rt_t=None, Tcb=None, stream=None):
        """airfe_frame_optimize_batch_dev: X_t / obs_t [B,ncap,3] float64, n_t [B] int32, Twc0_t [B,16] float64 -> Twc_t [B,16] float64,
        inlier_t [B,ncap] uint8, num_t [B] int32, Rt_t [B,12] float64 (optional).  Asynchronous on `stream`."""
        cam = np.ascontiguousarray(cam, np.float64).reshape(5)
        thr = np.ascontiguousarray(thr, np.float64).reshape(2)
        keep, tcb = self._tcb(Tcb)
        self._chk(self._l.airfe_frame_optimize_batch_dev(self._h, X_t.data_ptr(), obs_t.data_ptr(), n_t.data_ptr(), X_t.shape[0], X_t.shape[1],
                                                         Twc0_t.data_ptr(), cam.ctypes.data, tcb, thr.ctypes.data, Twc_t.data_ptr(),
                                                         None if Rt_t is None else Rt_t.data_ptr(), inlier_t.data_ptr(), num_t.data_ptr(),
                                                         self._stream(stream)), "airfe_frame_optimize_batch_dev")

    def track_pose_opt_batch_dev(self, cam, thr, lost_num_match, xyz_t, feat_t, tidx_t, ntrack_t, Twc_t, mask_t, num_t, ok_t, u_right_t=None,
                                 Twc_last_t=None, Rt_t=None, pnp_count_t=None, stream=None):
        """airfe_track_pose_opt_batch_dev (FramePoseOptimization without IMU, map_builder.cc:307-317, 353-417): the inputs of track_pose_batch_dev plus
        u_right_t [B,cap] float64 of the current frame (None: all mono), Twc_last_t [B,16] (None: identity), lost_num_match, cam = (fx, fy, cx, cy, bf),
        thr -> Twc_t [B,16], mask_t [B,mcap] uint8 (per list entry), num_t [B], ok_t [B] int32, Rt_t [B,12], pnp_count_t [B] (optional)."""
        cam = np.ascontiguousarray(cam, np.float64).reshape(5)
        thr = np.ascontiguousarray(thr, np.float64).reshape(2)
        opt = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        self._chk(self._l.airfe_track_pose_opt_batch_dev(self._h, cam.ctypes.data, thr.ctypes.data, int(lost_num_match), xyz_t.data_ptr(), xyz_t.shape[1],
                                                         feat_t.data_ptr(), feat_t.shape[1], tidx_t.data_ptr(), ntrack_t.data_ptr(), tidx_t.shape[1],
                                                         tidx_t.shape[0], opt(u_right_t), opt(Twc_last_t), Twc_t.data_ptr(), opt(Rt_t), mask_t.data_ptr(),
                                                         num_t.data_ptr(), ok_t.data_ptr(), opt(pnp_count_t), self._stream(stream)),
                  "airfe_track_pose_opt_batch_dev")

    def match_lightglue_batch_dev(self, f0_t, n0_t, f1_t, n1_t, idx_t, score_t, nm_t, stream=None):
        self._chk(self._l.airfe_match_lightglue_batch_dev(self._h, f0_t.data_ptr(), n0_t.data_ptr(), f1_t.data_ptr(),
                                                          n1_t.data_ptr(), f0_t.shape[0], f0_t.shape[1], idx_t.data_ptr(),
                                                          score_t.data_ptr(), idx_t.shape[1], nm_t.data_ptr(), self._stream(stream)),
                  "airfe_match_lightglue_batch_dev")

    def match_superglue_batch_dev(self, f0_t, n0_t, f1_t, n1_t, idx0_t, idx1_t, ms0_t, ms1_t, stream=None):
        self._chk(self._l.airfe_match_superglue_batch_dev(self._h, f0_t.data_ptr(), n0_t.data_ptr(), f1_t.data_ptr(), n1_t.data_ptr(),
                                                          f0_t.shape[0], f0_t.shape[1], idx0_t.data_ptr(), idx1_t.data_ptr(),
                                                          ms0_t.data_ptr(), ms1_t.data_ptr(), self._stream(stream)),
                  "airfe_match_superglue_batch_dev")

    def stereo_batch_dev(self, left_t, right_t, featL, featR, nL, nR, idx_t, score_t, nm_t, stream=None):
        b, h, w = left_t.shape
        self._chk(self._l.airfe_stereo_batch_dev(self._h, left_t.data_ptr(), right_t.data_ptr(), b, h, w, left_t.stride(1),
                                                 left_t.stride(0), featL.data_ptr(), featR.data_ptr(), featL.shape[1],
                                                 nL.data_ptr(), nR.data_ptr(), idx_t.data_ptr(), score_t.data_ptr(),
                                                 idx_t.shape[1], nm_t.data_ptr(), self._stream(stream)), "airfe_stereo_batch_dev")

    def detect_plnet_batch_dev(self, gray_t, feat_t, n_t, lines_t, nlines_t, junc_t=None, njunc_t=None, found_t=None, stream=None):
        """PLNet over a device batch: gray [B][h][w] u8, feat [B][cap][259] f32, n [B] i32, lines [B][capL][4] f64, nlines [B] i32,
        junc [J][capJ][259] f32 + njunc [J] i32 for the first J images (None: no junctions), found [B + J] i32 (None: not reported)."""
        b, h, w = gray_t.shape
        nj = 0 if junc_t is None else junc_t.shape[0]
        self._chk(self._l.airfe_detect_plnet_batch_dev(
            self._h, gray_t.data_ptr(), b, h, w, gray_t.stride(1), gray_t.stride(0), feat_t.data_ptr(), feat_t.shape[1], n_t.data_ptr(),
            lines_t.data_ptr(), lines_t.shape[1], nlines_t.data_ptr(), junc_t.data_ptr() if nj else None, junc_t.shape[1] if nj else 0,
            njunc_t.data_ptr() if nj else None, nj, found_t.data_ptr() if found_t is not None else None, self._stream(stream)),
            "airfe_detect_plnet_batch_dev")

    def stereo_plnet_batch_dev(self, left_t, right_t, featL, featR, nL, nR, lines_t, nlines_t, juncL, njuncL, idx_t, score_t, nm_t,
                               found_t=None, stream=None):
        """B stereo pairs with the PLNet detector: lines [2B][capL][4] / nlines [2B] (left images first), junctions of the left images
        juncL [B][capJ][259] / njuncL [B], LightGlue matches as stereo_batch_dev; found [3B] i32 (None: not reported)."""
        b, h, w = left_t.shape
        self._chk(self._l.airfe_stereo_plnet_batch_dev(
            self._h, left_t.data_ptr(), right_t.data_ptr(), b, h, w, left_t.stride(1), left_t.stride(0), featL.data_ptr(), featR.data_ptr(),
            featL.shape[1], nL.data_ptr(), nR.data_ptr(), lines_t.data_ptr(), lines_t.shape[1], nlines_t.data_ptr(), juncL.data_ptr(),
            juncL.shape[1], njuncL.data_ptr(), found_t.data_ptr() if found_t is not None else None, idx_t.data_ptr(), score_t.data_ptr(),
            idx_t.shape[1], nm_t.data_ptr(), self._stream(stream)), "airfe_stereo_plnet_batch_dev")

    def assign_points_to_lines_batch_dev(self, lines_t, nlines_t, feat_t, n_t, row_ptr_t, pt_idx_t, pt_dist_t, total_t=None, stream=None):
        """AssignPointsToLines (src/line_processor.cc:68-120) over B device-resident frames: lines [B][capL][4] f64 + nlines [B], feat [B][cap][259] + n [B]
        -> CSR per frame row_ptr [B][capL + 1] i32, pt_idx [B][capE] i32, pt_dist [B][capE] f64, total [B] i32 (entries found; > capE = overflow)."""
        b, capl = lines_t.shape[0], lines_t.shape[1]
        self._chk(self._l.airfe_assign_points_to_lines_batch_dev(
            self._h, lines_t.data_ptr(), nlines_t.data_ptr(), capl, feat_t.data_ptr(), n_t.data_ptr(), feat_t.shape[1], b, row_ptr_t.data_ptr(),
            pt_idx_t.data_ptr(), pt_dist_t.data_ptr(), pt_idx_t.shape[1], total_t.data_ptr() if total_t is not None else None, self._stream(stream)),
            "airfe_assign_points_to_lines_batch_dev")

    def match_lines_batch_dev(self, row_ptr0_t, pt_idx0_t, nlines0_t, n0_t, row_ptr1_t, pt_idx1_t, nlines1_t, n1_t, matches_t, nmatch_t, line_matches_t,
                              stereo_filter=None, feat0_t=None, feat1_t=None, stream=None):
        """MatchLines (src/line_processor.cc:122-180) over B frame pairs from the relations above and the matcher's lists matches [B][mcap][2] / nmatch [B]
        -> line_matches [B][capL] i32.  stereo_filter = (min_x_diff, max_x_diff, max_y_diff): the band of Frame::AddRightFeatures (src/frame.cc:147-160)."""
        b, capl = line_matches_t.shape
        f3 = (C.c_double * 3)(*stereo_filter) if stereo_filter is not None else None
        self._chk(self._l.airfe_match_lines_batch_dev(
            self._h, row_ptr0_t.data_ptr(), pt_idx0_t.data_ptr(), nlines0_t.data_ptr(), n0_t.data_ptr(), row_ptr1_t.data_ptr(), pt_idx1_t.data_ptr(),
            nlines1_t.data_ptr(), n1_t.data_ptr(), capl, pt_idx0_t.shape[1], matches_t.data_ptr(), nmatch_t.data_ptr(), matches_t.shape[1], b,
            C.cast(f3, C.c_void_p) if f3 is not None else None, feat0_t.data_ptr() if feat0_t is not None else None,
            feat1_t.data_ptr() if feat1_t is not None else None, feat0_t.shape[1] if feat0_t is not None else 0, line_matches_t.data_ptr(),
            self._stream(stream)), "airfe_match_lines_batch_dev")

    def rectify_batch_dev(self, side, raw_t, rect_t, stream=None):
        """cv::remap of Camera::UndistortImage (camera.cc:161-182) over B device-resident raw images [B][h][w] u8 -> rect_t (same shape)."""
        b, h, w = raw_t.shape
        self._chk(self._l.airfe_rectify_batch_dev(self._h, side, raw_t.data_ptr(), b, h, w, raw_t.stride(1), raw_t.stride(0), rect_t.data_ptr(),
                                                  rect_t.stride(1), rect_t.stride(0), self._stream(stream)), "airfe_rectify_batch_dev")

    def bow_transform_dev(self, feat_t, word_t, weight_t, stream=None):
        """TemplatedVocabulary::transform per feature row of feat_t [..., 259] (device) -> word_t u32 / weight_t f32, one per row."""
        n = feat_t.numel() // FEAT
        self._chk(self._l.airfe_bow_transform_dev(self._h, feat_t.data_ptr(), n, word_t.data_ptr(), weight_t.data_ptr(), self._stream(stream)),
                  "airfe_bow_transform_dev")

    def bow_vector(self, feat_rows: np.ndarray, return_words: bool = False):
        """≙ Database::FrameToBow to its end (src/bow/database.cc:57-89) on one frame's rows [n, 259] -> (ids uint32 [nw], values float64 [nw]) in ascending
        word id, L1-normalised[, word_of_features uint32 [n]]."""
        f = np.ascontiguousarray(feat_rows, np.float32).reshape(-1, FEAT)
        n = f.shape[0]
        ids = np.empty((max(n, 1),), np.uint32); vals = np.empty((max(n, 1),), np.float64); words = np.empty((max(n, 1),), np.uint32)
        nw = C.c_int(0)
        self._chk(self._l.airfe_bow_vector(self._h, f.ctypes.data, n, ids.ctypes.data, vals.ctypes.data, C.byref(nw), words.ctypes.data), "airfe_bow_vector")
        out = (ids[:nw.value].copy(), vals[:nw.value].copy())
        return out + (words[:n].copy(),) if return_words else out

    def bow_vector_batch_dev(self, feat_t, n_t, ids_t, vals_t, nw_t, word_t=None, stream=None):
        """FrameToBow over B device frames: feat [B][cap][259] f32, n [B] i32 -> ids [B][cap] (int32 storage of the uint32 ids), vals [B][cap] f64, nw [B] i32,
        word [B][cap] or None (word_of_features)."""
        b, cap = feat_t.shape[0], feat_t.shape[1]
        self._chk(self._l.airfe_bow_vector_batch_dev(self._h, feat_t.data_ptr(), n_t.data_ptr(), b, cap, ids_t.data_ptr(), vals_t.data_ptr(), nw_t.data_ptr(),
                                                     word_t.data_ptr() if word_t is not None else None, self._stream(stream)), "airfe_bow_vector_batch_dev")

    def junction_connections(self, lines: np.ndarray, junc: np.ndarray, W: int, H: int, ecap: int = 4096):
        """≙ Frame::FindJunctionConnections (src/frame.cc:581-629), the host core on one frame: lines [nl, 4] f64, junction rows [nj, 259] ->
        (edges int32 [ne, 2] distinct, ascending by (a, b); per line (a, b) or (-1, -1) int32 [nl, 2]; status 0 / 2 = more than ecap edges)."""
        ln = np.ascontiguousarray(lines, np.float64).reshape(-1, 4)
        jn = np.ascontiguousarray(junc, np.float32).reshape(-1, FEAT)
        edge = np.zeros((max(int(ecap), 1), 2), np.int32)
        pair = np.zeros((max(len(ln), 1), 2), np.int32)
        ne = C.c_int(0)
        rc = self._l.airfe_junction_connections(self._h, ln.ctypes.data, len(ln), jn.ctypes.data, len(jn), int(W), int(H), edge.ctypes.data, int(ecap),
                                                C.byref(ne), pair.ctypes.data)
        if rc not in (0, 2):
            self._chk(rc, "airfe_junction_connections")
        return edge[:ne.value].copy(), pair[:len(ln)].copy(), rc

    def junction_connections_batch_dev(self, lines_t, nlines_t, junc_t, njunc_t, W, H, edge_t, nedge_t, status_t, line_pair_t=None, stream=None):
        """FindJunctionConnections over B device frames in place on the PLNet outputs: lines [B][capL][4] f64, nlines [B], junc [B][capJ][259], njunc [B] ->
        edge [B][ecap][2] i32, nedge [B], status [B], line_pair [B][capL][2] or None."""
        self._chk(self._l.airfe_junction_connections_batch_dev(
            self._h, lines_t.data_ptr(), nlines_t.data_ptr(), lines_t.shape[1], junc_t.data_ptr(), njunc_t.data_ptr(), junc_t.shape[1], junc_t.shape[0], int(W),
            int(H), edge_t.data_ptr(), edge_t.shape[1], nedge_t.data_ptr(), status_t.data_ptr(), line_pair_t.data_ptr() if line_pair_t is not None else None,
            self._stream(stream)), "airfe_junction_connections_batch_dev")

    def copy_rows_plan(self, jobs):
        """jobs: [(src tensor / pointer, dst tensor / pointer, count tensor (int32, one element) / pointer / None, row_bytes, cap rows)] -> a reusable plan for
        copy_rows_dev (the five host arrays of airfe_copy_rows_dev, built once: the buffers of a pipeline do not move)"""
        ptr = lambda x: 0 if x is None else (int(x) if isinstance(x, int) else x.data_ptr())        # (dst None: a plan for pack_rows_dev only)
        n = len(jobs)
        return dict(n=n, src=np.array([ptr(j[0]) for j in jobs], np.uint64), dst=np.array([ptr(j[1]) for j in jobs], np.uint64),
                    cnt=np.array([ptr(j[2]) for j in jobs], np.uint64), rb=np.array([j[3] for j in jobs], np.uint32), cap=np.array([j[4] for j in jobs], np.uint32),
                    keep=jobs)

    def copy_rows_dev(self, plan, stream=None):
        """airfe_copy_rows_dev: the valid rows of every job of `plan` in one launch on `stream` (asynchronous)"""
        self._chk(self._l.airfe_copy_rows_dev(self._h, plan["n"], plan["src"].ctypes.data, plan["dst"].ctypes.data, plan["cnt"].ctypes.data, plan["rb"].ctypes.data,
                                              plan["cap"].ctypes.data, self._stream(stream)), "airfe_copy_rows_dev")

    def pack_rows_dev(self, plan, packed_t, offsets_t, stream=None):
        """airfe_pack_rows_dev: the valid rows of every job of `plan` (its dst column is ignored) back to back into `packed_t` (device uint8), job j at
        offsets_t[j], offsets_t[n] = bytes used (device int64 [n + 1]); two launches on `stream` (asynchronous)"""
        assert offsets_t.numel() >= plan["n"] + 1
        self._chk(self._l.airfe_pack_rows_dev(self._h, plan["n"], plan["src"].ctypes.data, plan["cnt"].ctypes.data, plan["rb"].ctypes.data, plan["cap"].ctypes.data,
                                              packed_t.data_ptr(), offsets_t.data_ptr(), self._stream(stream)), "airfe_pack_rows_dev")

    def _stream(self, stream):
        # the ctx runs on its own non-blocking stream: order it after whatever torch queued on ITS streams
        if stream is None:
            import torch
            torch.cuda.synchronize()
        return stream

    def profile(self, on=True, stages=None):
        """Per-stage hipEvent timers: on=False off, on=True every stage, stages=[names] only those (cheaper)."""
        mask = 0
        if stages is not None:
            names = [self._l.airfe_profile_stage_name(i).decode() for i in range(self._l.airfe_profile_stages())]
            for s in stages:
                mask |= 1 << names.index(s)
        elif on:
            mask = -1
        self._chk(self._l.airfe_profile_enable(self._h, mask), "airfe_profile_enable")

    def profile_read(self):
        n = self._l.airfe_profile_stages()
        ms = (C.c_double * n)(); fl = (C.c_double * n)(); by = (C.c_double * n)(); la = (C.c_int * n)()
        self._chk(self._l.airfe_profile_read(self._h, ms, fl, by, la), "airfe_profile_read")
        return {self._l.airfe_profile_stage_name(i).decode(): dict(ms=ms[i], flops=fl[i], bytes=by[i], launches=la[i])
                for i in range(n)}

    def sync(self):
        self._chk(self._l.airfe_sync(self._h), "airfe_sync")

    def debug_fail_next_launch(self, stage):
        """stage: a profiling stage name (profile_read's keys) or None to disarm — see include/airfe_debug.h"""
        names = [self._l.airfe_profile_stage_name(i).decode() for i in range(self._l.airfe_profile_stages())]
        self._chk(self._l.airfe_debug_fail_next_launch(self._h, -1 if stage is None else names.index(stage)), "airfe_debug_fail_next_launch")

    # ---- fault hunting: checksums of the matcher's state behind every launch (airfe_debug_trace*)
    def trace(self, on=True):
        self._chk(self._l.airfe_debug_trace(self._h, 1 if on else 0), "airfe_debug_trace")

    def trace_stop(self, slot=-1):
        self._chk(self._l.airfe_debug_trace_stop(self._h, slot), "airfe_debug_trace_stop")

    def trace_buffer(self, slot, dtype):
        """The whole buffer slot `slot` of the last matcher call covers, as a flat numpy array of `dtype`."""
        _, _, units, uw = self.trace_slots()[slot]
        out = np.zeros(units * uw * 4 // np.dtype(dtype).itemsize, dtype)
        self._chk(self._l.airfe_debug_trace_buffer(self._h, slot, out.ctypes.data, out.nbytes), "airfe_debug_trace_buffer")
        return out

    def trace_slots(self):
        """[(name, first unit, units, words per unit)] of the last matcher call."""
        out = []
        for i in range(self._l.airfe_debug_trace_slots(self._h)):
            name = C.create_string_buffer(64)
            off, units, uw = C.c_uint(), C.c_uint(), C.c_uint()
            self._chk(self._l.airfe_debug_trace_slot(self._h, i, name, 64, C.byref(off), C.byref(units), C.byref(uw)), "airfe_debug_trace_slot")
            out.append((name.value.decode(), off.value, units.value, uw.value))
        return out

    def trace_read(self, table=False, stream=None):
        """(digests [slots] u64, unit table u64 or None) of the last matcher call; synchronises the stream."""
        slots = self.trace_slots()
        dig = np.zeros(len(slots), np.uint64)
        tab = np.zeros(slots[-1][1] + slots[-1][2], np.uint64) if (table and slots) else None
        self._chk(self._l.airfe_debug_trace_read(self._h, stream, dig.ctypes.data, tab.ctypes.data if tab is not None else None), "airfe_debug_trace_read")
        return dig, tab


class BowDatabase:
    """airfe_bowdb (include/airfe.h, "BoW keyframe database"): Database::AddFrame / Query / Score and the callers' sharing-word filters over keyframes
    that live on the device.  A frame's handle is its insertion index.  Owned by `ctx` (needs ctx.bow_load first); close() before the context's."""

    def __init__(self, ctx: Context, max_frames: int, cap: int, keep_features: bool = False):
        self._ctx, self._l = ctx, ctx._l
        self.max_frames, self.cap, self.keep_features = max_frames, cap, bool(keep_features)
        h = C.c_void_p()
        ctx._chk(self._l.airfe_bowdb_create(ctx._h, max_frames, cap, 1 if keep_features else 0, C.byref(h)), "airfe_bowdb_create")
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            self._l.airfe_bowdb_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def size(self) -> int:
        return self._l.airfe_bowdb_size(self._h)

    def clear(self):
        self._ctx._chk(self._l.airfe_bowdb_clear(self._h), "airfe_bowdb_clear")

    def add(self, ids: np.ndarray, vals: np.ndarray, nw: np.ndarray, feat: np.ndarray = None, n: np.ndarray = None):
        """host buffers: ids [B][cap] uint32, vals [B][cap] float64, nw [B] int32 (+ feat [B][cap][259] float32, n [B] int32 with keep_features)"""
        ids = np.ascontiguousarray(ids, np.uint32); vals = np.ascontiguousarray(vals, np.float64); nw = np.ascontiguousarray(nw, np.int32)
        feat = None if feat is None else np.ascontiguousarray(feat, np.float32)
        n = None if n is None else np.ascontiguousarray(n, np.int32)
        self._ctx._chk(self._l.airfe_bowdb_add(self._h, ids.ctypes.data, vals.ctypes.data, nw.ctypes.data, feat.ctypes.data if feat is not None else None,
                                               n.ctypes.data if n is not None else None, ids.shape[0], ids.shape[1]), "airfe_bowdb_add")

    def add_batch_dev(self, ids_t, vals_t, nw_t, feat_t=None, n_t=None, stream=None):
        """≙ Database::AddFrame for B device vectors (Context.bow_vector_batch_dev's outputs); asynchronous on `stream`"""
        self._ctx._chk(self._l.airfe_bowdb_add_batch_dev(self._h, ids_t.data_ptr(), vals_t.data_ptr(), nw_t.data_ptr(),
                                                         feat_t.data_ptr() if feat_t is not None else None, n_t.data_ptr() if n_t is not None else None,
                                                         ids_t.shape[0], ids_t.shape[1], self._ctx._stream(stream)), "airfe_bowdb_add_batch_dev")

    def query_batch_dev(self, ids_t, vals_t, nw_t, cand_frame_t, cand_sharing_t, cand_score_t, ncand_t, max_sharing_t, ratio=0.3, min_words=8,
                        max_index_t=None, exclude_t=None, sharing_t=None, stream=None):
        """Q query vectors [Q][cap] against every stored frame -> per query the candidates in ascending frame index: cand_frame / cand_sharing i32 [Q][ccap],
        cand_score f64 [Q][ccap], ncand [Q] (the full count), max_sharing [Q]; ratio 0.3 = relocalisation, 0.5 = loop detection; max_index [Q] i32 (frames
        below it only), exclude [Q][words] i32 bit rows, sharing [Q][size] i32 (dense counts), all optional."""
        from . import _lib
        f = _lib.BowdbFilter(float(ratio), int(min_words), max_index_t.data_ptr() if max_index_t is not None else None,
                             exclude_t.data_ptr() if exclude_t is not None else None, exclude_t.shape[1] if exclude_t is not None else 0)
        self._ctx._chk(self._l.airfe_bowdb_query_batch_dev(self._h, ids_t.data_ptr(), vals_t.data_ptr(), nw_t.data_ptr(), ids_t.shape[0], ids_t.shape[1], C.byref(f),
                                                           cand_frame_t.data_ptr(), cand_sharing_t.data_ptr(), cand_score_t.data_ptr(), cand_frame_t.shape[1],
                                                           ncand_t.data_ptr(), max_sharing_t.data_ptr(), sharing_t.data_ptr() if sharing_t is not None else None,
                                                           self._ctx._stream(stream)), "airfe_bowdb_query_batch_dev")

    def topk_dev(self, cand_frame_t, cand_score_t, ncand_t, top_t, top_score_t=None, stream=None):
        """the project's own ranking (not the reference's grouping): top [Q][K <= 8] i32 = the candidates by descending score, ties to the lower frame, -1 padded"""
        self._ctx._chk(self._l.airfe_bowdb_topk_dev(self._h, cand_frame_t.data_ptr(), cand_score_t.data_ptr(), ncand_t.data_ptr(), cand_frame_t.shape[0],
                                                    cand_frame_t.shape[1], top_t.shape[1], top_t.data_ptr(),
                                                    top_score_t.data_ptr() if top_score_t is not None else None, self._ctx._stream(stream)), "airfe_bowdb_topk_dev")

    def match_candidates_batch_dev(self, qfeat_t, qn_t, cand_t, best_t, idx_t, score_t, nmatch_t, nmatch_all_t=None, outlier_rejection=True, stream=None):
        """map_user.cc:360-376 / map_refiner.cc:213-230: every query [Q][cap][259] against its candidates cand [Q][K <= 5] (in order, -1 = none) through
        LightGlue (+ the F-matrix RANSAC) -> best [Q] (frame or -1), its list idx [Q][mcap][2] / score [Q][mcap] / nmatch [Q], nmatch_all [Q][K]."""
        self._ctx._chk(self._l.airfe_bowdb_match_candidates_batch_dev(
            self._ctx._h, self._h, qfeat_t.data_ptr(), qn_t.data_ptr(), qfeat_t.shape[0], qfeat_t.shape[1], cand_t.data_ptr(), cand_t.shape[1],
            1 if outlier_rejection else 0, best_t.data_ptr(), idx_t.data_ptr(), score_t.data_ptr(), idx_t.shape[1], nmatch_t.data_ptr(),
            nmatch_all_t.data_ptr() if nmatch_all_t is not None else None, self._ctx._stream(stream)), "airfe_bowdb_match_candidates_batch_dev")

    # ---- map state, the grouping and the relocalisation composite (include/airfe.h "Map state in the database", "Grouping", "Relocalisation composite")
    def attach_map(self, max_edges: int):
        """map points [max_frames][cap][3] (NaN = none), a covisibility table of up to max_edges entries and keyframe positions; needs keep_features"""
        self._ctx._chk(self._l.airfe_bowdb_attach_map(self._h, int(max_edges)), "airfe_bowdb_attach_map")

    def set_points(self, first_frame: int, xyz: np.ndarray):
        """host buffer xyz [B][cap][3] float64 (world frame; NaN where the row has no valid map point) -> frames first_frame .. first_frame + B - 1"""
        xyz = np.ascontiguousarray(xyz, np.float64).reshape(-1, self.cap, 3)
        self._ctx._chk(self._l.airfe_bowdb_set_points(self._h, int(first_frame), xyz.shape[0], xyz.ctypes.data), "airfe_bowdb_set_points")

    def set_points_dev(self, first_frame: int, xyz_t, stream=None):
        self._ctx._chk(self._l.airfe_bowdb_set_points_dev(self._h, int(first_frame), xyz_t.shape[0], xyz_t.data_ptr(), self._ctx._stream(stream)),
                       "airfe_bowdb_set_points_dev")

    def get_points(self, first_frame: int, B: int) -> np.ndarray:
        xyz = np.empty((B, self.cap, 3), np.float64)
        self._ctx._chk(self._l.airfe_bowdb_get_points(self._h, int(first_frame), B, xyz.ctypes.data), "airfe_bowdb_get_points")
        return xyz

    def set_covisibility(self, row_ptr: np.ndarray, nbr: np.ndarray, weight: np.ndarray):
        """replaces the whole graph: CSR over len(row_ptr) - 1 frames, every row strictly ascending in nbr, the frames' own entries included as the map has them"""
        row_ptr = np.ascontiguousarray(row_ptr, np.int32); nbr = np.ascontiguousarray(nbr, np.int32); weight = np.ascontiguousarray(weight, np.int32)
        if len(row_ptr) < 1 or len(nbr) != len(weight) or (len(nbr) and int(row_ptr[-1]) > len(nbr)):
            raise AirfeError("set_covisibility: row_ptr / nbr / weight do not describe one CSR table")
        self._ctx._chk(self._l.airfe_bowdb_set_covisibility(self._h, row_ptr.ctypes.data, nbr.ctypes.data if len(nbr) else None,
                                                            weight.ctypes.data if len(nbr) else None, len(row_ptr) - 1), "airfe_bowdb_set_covisibility")

    def get_covisibility(self, edge_cap: int):
        """-> (row_ptr [max_frames + 1], nbr [E], weight [E]) as the device holds them"""
        row_ptr = np.zeros(self.max_frames + 1, np.int32); nbr = np.zeros(max(edge_cap, 1), np.int32); weight = np.zeros(max(edge_cap, 1), np.int32)
        e = C.c_int(0)
        self._ctx._chk(self._l.airfe_bowdb_get_covisibility(self._h, row_ptr.ctypes.data, nbr.ctypes.data, weight.ctypes.data, int(edge_cap), C.byref(e)),
                       "airfe_bowdb_get_covisibility")
        return row_ptr, nbr[:e.value].copy(), weight[:e.value].copy()

    def set_positions(self, first_frame: int, pos: np.ndarray):
        """host buffer pos [B][3] float64: the keyframes' positions, read by the loop form of group_dev"""
        pos = np.ascontiguousarray(pos, np.float64).reshape(-1, 3)
        self._ctx._chk(self._l.airfe_bowdb_set_positions(self._h, int(first_frame), pos.shape[0], pos.ctypes.data), "airfe_bowdb_set_positions")

    def group_dev(self, mode, cand_frame_t, cand_score_t, ncand_t, group_frame_t, group_score_t, ngroups_t, status_t, extra_t=None, qpos_t=None,
                  max_dist_t=None, stream=None):
        """the grouping of map_user.cc:177-363 (mode 0, K <= 3) / map_refiner.cc:132-214 (mode 1, K <= 5) over query_batch_dev's candidate lists ->
        group_frame i32 [Q][K] (the deputies, -1 padded: match_candidates_batch_dev's cand), group_score f64 [Q][K], ngroups [Q], status [Q] (0 ok, 1 no
        group, 2 overflow); extra f64 [Q][size] (mode 0, optional), qpos f64 [Q][3] + max_dist f64 [Q] (mode 1)."""
        opt = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        self._ctx._chk(self._l.airfe_bowdb_group_dev(self._h, int(mode), cand_frame_t.data_ptr(), cand_score_t.data_ptr(), ncand_t.data_ptr(),
                                                     cand_frame_t.shape[0], cand_frame_t.shape[1], group_frame_t.shape[1], opt(extra_t), opt(qpos_t),
                                                     opt(max_dist_t), group_frame_t.data_ptr(), group_score_t.data_ptr(), ngroups_t.data_ptr(),
                                                     status_t.data_ptr(), self._ctx._stream(stream)), "airfe_bowdb_group_dev")

    def relocalize_batch_dev(self, qfeat_t, qn_t, cam, thr, min_inlier, ok_t, stage_t, Twc_t, best_t, num_t, mask_t, idx_t, score_t, nmatch_t,
                             pnp_count_t=None, extra_t=None, pose_refinement=True, K=3, ratio=0.3, min_words=8, outlier_rejection=True, stream=None):
        """airfe_relocalize_batch_dev (map_user.cc:129-460): qfeat [Q][cap][259] + qn [Q] -> ok / stage [Q] i32, Twc [Q][16] f64, best [Q], num [Q],
        mask [Q][mcap] u8 by list entry, the winner's list idx [Q][mcap][2] / score [Q][mcap] / nmatch [Q], pnp_count [Q] (optional)."""
        from . import _lib
        cfg = _lib.RelocCfg(float(ratio), int(min_words), int(K), 1 if outlier_rejection else 0, int(min_inlier), 1 if pose_refinement else 0,
                            (C.c_double * 5)(*[float(x) for x in cam]), (C.c_double * 2)(*[float(x) for x in thr]))
        opt = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        self._ctx._chk(self._l.airfe_relocalize_batch_dev(
            self._ctx._h, self._h, C.byref(cfg), qfeat_t.data_ptr(), qn_t.data_ptr(), qfeat_t.shape[0], qfeat_t.shape[1], opt(extra_t), ok_t.data_ptr(),
            stage_t.data_ptr(), Twc_t.data_ptr(), best_t.data_ptr(), num_t.data_ptr(), mask_t.data_ptr(), idx_t.data_ptr(), score_t.data_ptr(), idx_t.shape[1],
            nmatch_t.data_ptr(), opt(pnp_count_t), self._ctx._stream(stream)), "airfe_relocalize_batch_dev")

    # ---- loop detection over a loaded map (include/airfe.h "Map state for loop detection", "Stored queries against their predecessors", "Loop detection
    # composite")
    def set_poses(self, first_frame: int, Twc: np.ndarray):
        """host buffer Twc [B][16] (or [B][4][4]) float64 row-major -> the pose table; the translation columns also become the positions group_dev reads"""
        Twc = np.ascontiguousarray(Twc, np.float64).reshape(-1, 16)
        self._ctx._chk(self._l.airfe_bowdb_set_poses(self._h, int(first_frame), Twc.shape[0], Twc.ctypes.data), "airfe_bowdb_set_poses")

    def get_poses(self, first_frame: int, B: int) -> np.ndarray:
        Twc = np.empty((B, 16), np.float64)
        self._ctx._chk(self._l.airfe_bowdb_get_poses(self._h, int(first_frame), B, Twc.ctypes.data), "airfe_bowdb_get_poses")
        return Twc

    def set_u_right(self, first_frame: int, u_right: np.ndarray):
        """host buffer u_right [B][cap] float64: the stored frames' right-image columns (> 0: the row has a stereo match)"""
        u_right = np.ascontiguousarray(u_right, np.float64).reshape(-1, self.cap)
        self._ctx._chk(self._l.airfe_bowdb_set_u_right(self._h, int(first_frame), u_right.shape[0], u_right.ctypes.data), "airfe_bowdb_set_u_right")

    def set_u_right_dev(self, first_frame: int, u_right_t, stream=None):
        self._ctx._chk(self._l.airfe_bowdb_set_u_right_dev(self._h, int(first_frame), u_right_t.shape[0], u_right_t.data_ptr(), self._ctx._stream(stream)),
                       "airfe_bowdb_set_u_right_dev")

    def get_u_right(self, first_frame: int, B: int) -> np.ndarray:
        u = np.empty((B, self.cap), np.float64)
        self._ctx._chk(self._l.airfe_bowdb_get_u_right(self._h, int(first_frame), B, u.ctypes.data), "airfe_bowdb_get_u_right")
        return u

    def query_stored_batch_dev(self, qframe_t, cand_frame_t, cand_sharing_t, cand_score_t, ncand_t, max_sharing_t, ratio=0.5, min_words=8,
                               exclude_covisible=False, sharing_t=None, stream=None):
        """map_refiner.cc:95-130 for stored frames qframe [Q] i32: frame fq against frames 0 .. fq - 1 only (max_sharing and the threshold over that prefix),
        optionally without its covisible frames -> query_batch_dev's outputs; sharing [Q][size] i32 (dense counts, 0 from fq on), optional."""
        self._ctx._chk(self._l.airfe_bowdb_query_stored_batch_dev(
            self._h, qframe_t.data_ptr(), qframe_t.shape[0], float(ratio), int(min_words), 1 if exclude_covisible else 0, cand_frame_t.data_ptr(),
            cand_sharing_t.data_ptr(), cand_score_t.data_ptr(), cand_frame_t.shape[1], ncand_t.data_ptr(), max_sharing_t.data_ptr(),
            sharing_t.data_ptr() if sharing_t is not None else None, self._ctx._stream(stream)), "airfe_bowdb_query_stored_batch_dev")

    def loop_detect_batch_dev(self, qframe_t, cam, thr, ok_t, stage_t, loop_t, Twq_t, Rlq_t, tlq_t, num_t, mask_t, idx_t, score_t, nmatch_t, ncons_t=None,
                              K=5, ratio=0.5, min_words=8, outlier_rejection=True, distance_rate=0.03, min_matches=50, min_points=50, min_inliers=50,
                              stream=None):
        """airfe_loop_detect_batch_dev (map_refiner.cc:65-333): stored frames qframe [Q] i32 -> ok / stage [Q] i32, loop [Q] i32 (the loop frame or -1),
        Twq [Q][16], Rlq [Q][9], tlq [Q][3] f64, num [Q], mask [Q][mcap] u8 by list entry, the winner's list idx [Q][mcap][2] / score [Q][mcap] /
        nmatch [Q], ncons [Q] (optional)."""
        from . import _lib
        cfg = _lib.LoopCfg(float(ratio), int(min_words), int(K), 1 if outlier_rejection else 0, float(distance_rate), int(min_matches), int(min_points),
                           int(min_inliers), (C.c_double * 5)(*[float(x) for x in cam]), (C.c_double * 2)(*[float(x) for x in thr]))
        self._ctx._chk(self._l.airfe_loop_detect_batch_dev(
            self._ctx._h, self._h, C.byref(cfg), qframe_t.data_ptr(), qframe_t.shape[0], ok_t.data_ptr(), stage_t.data_ptr(), loop_t.data_ptr(),
            Twq_t.data_ptr(), Rlq_t.data_ptr(), tlq_t.data_ptr(), num_t.data_ptr(), mask_t.data_ptr(), idx_t.data_ptr(), score_t.data_ptr(), idx_t.shape[1],
            nmatch_t.data_ptr(), ncons_t.data_ptr() if ncons_t is not None else None, self._ctx._stream(stream)), "airfe_loop_detect_batch_dev")


    # ---- map-point ids and the covisibility build (include/airfe.h "Map-point ids and the covisibility build")
    def attach_point_ids(self, max_points: int):
        """the id table [max_frames][cap] int32 (-1 everywhere) and the build's work arrays for ids 0 .. max_points - 1; needs attach_map"""
        self._ctx._chk(self._l.airfe_bowdb_attach_point_ids(self._h, int(max_points)), "airfe_bowdb_attach_point_ids")

    def set_point_ids(self, first_frame: int, ids: np.ndarray):
        """host buffer ids [B][cap] int32: the map point at each feature row, -1 where there is none (the rows that hold NaN in the point table)"""
        ids = np.ascontiguousarray(ids, np.int32).reshape(-1, self.cap)
        self._ctx._chk(self._l.airfe_bowdb_set_point_ids(self._h, int(first_frame), ids.shape[0], ids.ctypes.data), "airfe_bowdb_set_point_ids")

    def set_point_ids_dev(self, first_frame: int, ids_t, stream=None):
        self._ctx._chk(self._l.airfe_bowdb_set_point_ids_dev(self._h, int(first_frame), ids_t.shape[0], ids_t.data_ptr(), self._ctx._stream(stream)),
                       "airfe_bowdb_set_point_ids_dev")

    def get_point_ids(self, first_frame: int, B: int) -> np.ndarray:
        ids = np.empty((B, self.cap), np.int32)
        self._ctx._chk(self._l.airfe_bowdb_get_point_ids(self._h, int(first_frame), B, ids.ctypes.data), "airfe_bowdb_get_point_ids")
        return ids

    def build_covisibility_dev(self, info_t, stream=None):
        """Map::UpdateCovisibilityGraph from the id table, asynchronous on `stream`: replaces the whole graph; info i32 [4] (device) = status (1: more
        entries than max_edges, the graph is empty), entries needed, valid (frame, row) entries, ids ignored as out of range"""
        self._ctx._chk(self._l.airfe_bowdb_build_covisibility_dev(self._h, info_t.data_ptr(), self._ctx._stream(stream)), "airfe_bowdb_build_covisibility_dev")

    def build_covisibility(self) -> int:
        """the same on the context's stream, then a synchronisation -> the number of entries; more than max_edges raises (the graph is empty then)"""
        e = C.c_int(0)
        self._ctx._chk(self._l.airfe_bowdb_build_covisibility(self._h, C.byref(e)), "airfe_bowdb_build_covisibility")
        return e.value

    # ---- map-point triangulation (include/airfe.h "Map-point triangulation")
    @staticmethod
    def _cam4(cam):
        return (C.c_double * 4)(*[float(x) for x in cam])

    def attach_triangulation(self):
        """the observation segments and the host form's outputs; needs attach_point_ids; nothing is allocated afterwards"""
        self._ctx._chk(self._l.airfe_bowdb_attach_triangulation(self._h), "airfe_bowdb_attach_triangulation")

    def triangulate_points_dev(self, cam, xyz_t, status_t, nobs_t, info_t, min_observers=2, stream=None):
        """Map::TriangulateMappoint for every point of the id table from the stored rows and poses, asynchronous on `stream`: cam = (fx, fy, cx, cy);
        xyz f64 [max_points][3] (NaN unless status is 0), status / nobs i32 [max_points], info i32 [4] = ok, observed, status 2, status 3"""
        self._ctx._chk(self._l.airfe_bowdb_triangulate_points_dev(
            self._h, None if cam is None else self._cam4(cam), int(min_observers), xyz_t.data_ptr() if xyz_t is not None else None,
            status_t.data_ptr() if status_t is not None else None, nobs_t.data_ptr() if nobs_t is not None else None,
            info_t.data_ptr() if info_t is not None else None, self._ctx._stream(stream)), "airfe_bowdb_triangulate_points_dev")

    def triangulate_points(self, cam, max_points: int, min_observers=2):
        """the same into host buffers on the context's stream, then a synchronisation -> (xyz [max_points][3], status, nobs, the points of status 0);
        max_points: attach_point_ids'"""
        xyz = np.empty((max_points, 3), np.float64); status = np.empty(max_points, np.int32); nobs = np.empty(max_points, np.int32)
        ok = C.c_int(0)
        self._ctx._chk(self._l.airfe_bowdb_triangulate_points(self._h, self._cam4(cam), int(min_observers), xyz.ctypes.data, status.ctypes.data,
                                                              nobs.ctypes.data, C.byref(ok)), "airfe_bowdb_triangulate_points")
        return xyz, status, nobs, ok.value

    def fill_points_dev(self, xyz_t, status_t, written_t, only_missing=False, stream=None):
        """points[f][i] = xyz[id] for every valid row whose point has status 0 (only_missing: only where the stored x is NaN); written i32 [1]"""
        self._ctx._chk(self._l.airfe_bowdb_fill_points_dev(
            self._h, xyz_t.data_ptr() if xyz_t is not None else None, status_t.data_ptr() if status_t is not None else None, 1 if only_missing else 0,
            written_t.data_ptr() if written_t is not None else None, self._ctx._stream(stream)), "airfe_bowdb_fill_points_dev")

    def retriangulate_dev(self, cam, xyz_t, status_t, nobs_t, info_t, written_t, min_observers=2, only_missing=False, stream=None):
        """triangulate_points_dev, then fill_points_dev with its outputs, on one stream: the point table brought in line with the poses"""
        self.triangulate_points_dev(cam, xyz_t, status_t, nobs_t, info_t, min_observers=min_observers, stream=stream)
        self.fill_points_dev(xyz_t, status_t, written_t, only_missing=only_missing, stream=stream)

    # ---- map-point merge (include/airfe.h "Map-point merge")
    def attach_merge(self):
        """the merge's work arrays (24 bytes per point, 4 per feature row); needs attach_point_ids; nothing is allocated by a _dev call afterwards"""
        self._ctx._chk(self._l.airfe_bowdb_attach_merge(self._h), "airfe_bowdb_attach_merge")

    def merge_points_dev(self, pairs_t, map_t, info_t, stream=None):
        """MergeMappoints on an explicit pair list pairs i32 [P][2] (device), asynchronous on `stream`: the id table and the point table are relabelled in
        place; map i32 [max_points] = the best of an id's group or the id itself; info i32 [8] = pairs taken, pairs ignored, 0, 0, groups, ids removed,
        rows relabelled, rows cleared"""
        P = 0 if pairs_t is None else int(pairs_t.shape[0])
        self._ctx._chk(self._l.airfe_bowdb_merge_points_dev(
            self._h, pairs_t.data_ptr() if P else None, P, map_t.data_ptr() if map_t is not None else None,
            info_t.data_ptr() if info_t is not None else None, self._ctx._stream(stream)), "airfe_bowdb_merge_points_dev")

    def merge_points(self, pairs: np.ndarray, max_points: int):
        """the same from a host pair list on the context's stream, then a synchronisation -> (map [max_points], info [8]); max_points: attach_point_ids'"""
        pairs = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
        mp, info = np.empty(max_points, np.int32), np.empty(8, np.int32)
        self._ctx._chk(self._l.airfe_bowdb_merge_points(self._h, pairs.ctypes.data if len(pairs) else None, len(pairs), mp.ctypes.data, info.ctypes.data),
                       "airfe_bowdb_merge_points")
        return mp, info

    def loop_merge_batch_dev(self, cam, qframe_t, stage_t, loop_t, Rlq_t, tlq_t, mask_t, idx_t, nmatch_t, map_t, info_t, stream=None):
        """The tail of RelativatePoseEstimation and MergeMappoints straight from loop_detect_batch_dev's buffers, asynchronous on `stream`: cam = (fx, fy,
        cx, cy); live entries adopt or pair, groups are merged into their best, the id table and the point table are relabelled in place; map i32
        [max_points]; info i32 [8] = live, outliers, epipolar, rows adopted, groups, ids removed, rows relabelled, rows cleared"""
        Q = int(qframe_t.shape[0])
        p = lambda t: t.data_ptr() if (t is not None and Q) else None  # noqa: E731
        self._ctx._chk(self._l.airfe_bowdb_loop_merge_batch_dev(
            self._h, None if cam is None else self._cam4(cam), p(qframe_t), Q, p(stage_t), p(loop_t), p(Rlq_t), p(tlq_t), p(mask_t), p(idx_t),
            int(idx_t.shape[1]), p(nmatch_t), map_t.data_ptr() if map_t is not None else None, info_t.data_ptr() if info_t is not None else None,
            self._ctx._stream(stream)), "airfe_bowdb_loop_merge_batch_dev")

    def loop_close_dev(self, cam, qframe_t, stage_t, loop_t, Rlq_t, tlq_t, mask_t, idx_t, nmatch_t, map_t, merge_info_t, xyz_t, status_t, nobs_t, tri_info_t,
                       written_t, covis_info_t, min_observers=2, stream=None):
        """loop_merge_batch_dev, then retriangulate_dev(only_missing=True), then build_covisibility_dev, on one stream: a detected loop taken into the map"""
        self.loop_merge_batch_dev(cam, qframe_t, stage_t, loop_t, Rlq_t, tlq_t, mask_t, idx_t, nmatch_t, map_t, merge_info_t, stream=stream)
        self.retriangulate_dev(cam, xyz_t, status_t, nobs_t, tri_info_t, written_t, min_observers=min_observers, only_missing=True, stream=stream)
        self.build_covisibility_dev(covis_info_t, stream=stream)


# ------------------------------------------------------------------------------------ reference-shaped façade
    # ---- the junction term (include/airfe.h "Junction term"): this database is the JUNCTION database, frame f = frame f of the point database
    def attach_junctions(self, ecap: int, max_queries: int):
        """allocates the stored frames' words and tables, the queries' tables and the composites' chain; nothing is allocated afterwards"""
        self._ctx._chk(self._l.airfe_bowdb_attach_junctions(self._h, int(ecap), int(max_queries)), "airfe_bowdb_attach_junctions")
        self._ecap = int(ecap)

    def set_junctions_dev(self, first_frame: int, word_t, nj_t, edge_t, nedge_t, status_t=None, stream=None):
        """word [B][cap] (uint32 in int32 storage), nj [B], edge [B][ecap][2], nedge [B], status [B] or None, on the device"""
        self._ctx._chk(self._l.airfe_bowdb_set_junctions_dev(self._h, int(first_frame), word_t.shape[0], word_t.data_ptr(), nj_t.data_ptr(), edge_t.data_ptr(),
                                                             nedge_t.data_ptr(), status_t.data_ptr() if status_t is not None else None,
                                                             self._ctx._stream(stream)), "airfe_bowdb_set_junctions_dev")

    def set_junctions(self, first_frame: int, word: np.ndarray, nj: np.ndarray, edge: np.ndarray, nedge: np.ndarray, status: np.ndarray = None):
        """the same on host buffers; at most max_queries frames per call"""
        word = np.ascontiguousarray(word, np.uint32); nj = np.ascontiguousarray(nj, np.int32)
        edge = np.ascontiguousarray(edge, np.int32); nedge = np.ascontiguousarray(nedge, np.int32)
        status = None if status is None else np.ascontiguousarray(status, np.int32)
        self._ctx._chk(self._l.airfe_bowdb_set_junctions(self._h, int(first_frame), word.shape[0], word.ctypes.data, nj.ctypes.data, edge.ctypes.data,
                                                         nedge.ctypes.data, status.ctypes.data if status is not None else None), "airfe_bowdb_set_junctions")

    def get_junctions(self, first_frame: int, B: int, cap: int, ecap: int) -> dict:
        """-> dict(word, nj, uword, wcnt, wconn, nuw, ukey, kcnt, nuk, status) of frames first_frame .. (entries past nuw / nuk are not meaningful)"""
        o = dict(word=np.zeros((B, cap), np.uint32), nj=np.zeros(B, np.int32), uword=np.zeros((B, cap), np.uint32), wcnt=np.zeros((B, cap), np.int32),
                 wconn=np.zeros((B, cap), np.int32), nuw=np.zeros(B, np.int32), ukey=np.zeros((B, ecap), np.uint64), kcnt=np.zeros((B, ecap), np.int32),
                 nuk=np.zeros(B, np.int32), status=np.zeros(B, np.int32))
        self._ctx._chk(self._l.airfe_bowdb_get_junctions(self._h, int(first_frame), int(B), *[o[k].ctypes.data for k in (
            "word", "nj", "uword", "wcnt", "wconn", "nuw", "ukey", "kcnt", "nuk", "status")]), "airfe_bowdb_get_junctions")
        return o

    def junction_term_batch_dev(self, ids_t, vals_t, nw_t, word_t, nj_t, edge_t, nedge_t, extra_t, qstatus_t=None, match_num_t=None, line_match_num_t=None,
                                stream=None):
        """≙ map_user.cc:290-331 for Q queries against every stored frame: the queries' junction vectors and words (bow_vector_batch_dev on this database's
        context), their connections -> extra f64 [Q][N], match_num / line_match_num i32 [Q][N] or None"""
        p = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
        self._ctx._chk(self._l.airfe_bowdb_junction_term_batch_dev(self._h, ids_t.data_ptr(), vals_t.data_ptr(), nw_t.data_ptr(), word_t.data_ptr(), nj_t.data_ptr(),
                                                                   edge_t.data_ptr(), nedge_t.data_ptr(), p(qstatus_t), ids_t.shape[0], extra_t.data_ptr(),
                                                                   p(match_num_t), p(line_match_num_t), self._ctx._stream(stream)),
                       "airfe_bowdb_junction_term_batch_dev")

    def junction_extra_batch_dev(self, junc_t, njunc_t, lines_t, nlines_t, W, H, extra_t, match_num_t=None, line_match_num_t=None, stream=None):
        """the composite: the query frames' junction rows [Q][capJ][259] and lines [Q][capL][4] -> extra [Q][N] for relocalize_batch_dev, on one stream"""
        p = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
        self._ctx._chk(self._l.airfe_bowdb_junction_extra_batch_dev(self._h, junc_t.data_ptr(), njunc_t.data_ptr(), junc_t.shape[1], lines_t.data_ptr(),
                                                                    nlines_t.data_ptr(), lines_t.shape[1], junc_t.shape[0], int(W), int(H), extra_t.data_ptr(),
                                                                    p(match_num_t), p(line_match_num_t), self._ctx._stream(stream)),
                       "airfe_bowdb_junction_extra_batch_dev")

    def add_junction_frames_batch_dev(self, junc_t, njunc_t, lines_t, nlines_t, W, H, stream=None):
        """≙ BuildJunctionDatabase's second loop + FindJunctionConnections (map_refiner.cc:977, 986-994) for B map frames: vector, add, connections, tables"""
        self._ctx._chk(self._l.airfe_bowdb_add_junction_frames_batch_dev(self._h, junc_t.data_ptr(), njunc_t.data_ptr(), junc_t.shape[1], lines_t.data_ptr(),
                                                                         nlines_t.data_ptr(), lines_t.shape[1], junc_t.shape[0], int(W), int(H),
                                                                         self._ctx._stream(stream)), "airfe_bowdb_add_junction_frames_batch_dev")


def triangulate_point(cam, Twc: np.ndarray, xy: np.ndarray):
    """airfe_triangulate_point: Map::TriangulateMappoint for one point on the host, without a context.  cam = (fx, fy, cx, cy), Twc [n][16] (or [n][4][4])
    float64, xy [n][2] float32 in observer order -> (xyz [3], status); at least two observers (include/airfe.h "Map-point triangulation")."""
    l = _lib.lib()
    Twc = np.ascontiguousarray(Twc, np.float64).reshape(-1, 16)
    xy = np.ascontiguousarray(xy, np.float32).reshape(-1, 2)
    if len(Twc) != len(xy):
        raise AirfeError("triangulate_point: Twc and xy differ in length")
    xyz = np.empty(3, np.float64)
    status = C.c_int(0)
    if l.airfe_triangulate_point((C.c_double * 4)(*[float(x) for x in cam]), Twc.ctypes.data, xy.ctypes.data, len(xy), xyz.ctypes.data, C.byref(status)) != 0:
        raise AirfeError(f"airfe_triangulate_point: {(l.airfe_last_error(None) or b'').decode()}")
    return xyz, status.value


class FeatureDetector:
    """Mirror of FeatureDetector (include/feature_detector.h:8-31, src/feature_detector.cc)."""

    def __init__(self, ctx: Context):
        self._ctx = ctx

    def Detect(self, image: np.ndarray):
        """Detect(cv::Mat&, Eigen::Matrix<float,259,Dynamic>&) -> (ok, features [259, N])."""
        try:
            f = self._ctx.detect_points(image)
        except (AirfeError, TypeError):
            print("Failed when extracting point features !")     # feature_detector.cc:46-48
            return False, np.zeros((FEAT, 0), np.float32, order="F")
        return True, np.asfortranarray(f.T)

    def DetectLines(self, image: np.ndarray, stage0, lines: list, junction_detection: bool = False):
        """Detect(image, features, lines[, junctions]) (feature_detector.cc:52-69) -> (ok, features, junctions).
        `lines` is APPENDED to, never cleared — exactly like the reference (plnet.cpp:544)."""
        try:
            f, l, j = self._ctx.detect_plnet(image, stage0, want_junctions=junction_detection)
        except (AirfeError, TypeError):
            print("Failed when extracting point features !")
            return False, np.zeros((FEAT, 0), np.float32, order="F"), np.zeros((FEAT, 0), np.float32, order="F")
        lines.extend(tuple(r) for r in l)
        return True, np.asfortranarray(f.T), np.asfortranarray(j.T)

    def DetectKeyframe(self, left: np.ndarray, right: np.ndarray, left_lines: list, right_lines: list):
        """Detect(image_left, image_right, left_features, right_features, left_lines, right_lines, junctions) (feature_detector.cc:97-108) as ONE
        device pass over both images (Context.stereo_keyframe without the match) -> (ok, left_features, right_features, junctions)."""
        try:
            k = self._ctx.stereo_keyframe(left, right, match=False)
        except (AirfeError, TypeError):
            print("Failed when extracting point features !")
            z = np.zeros((FEAT, 0), np.float32, order="F")
            return False, z, z.copy(), z.copy()
        left_lines.extend(tuple(r) for r in k["linesL"])
        right_lines.extend(tuple(r) for r in k["linesR"])
        return True, np.asfortranarray(k["featL"].T), np.asfortranarray(k["featR"].T), np.asfortranarray(k["juncL"].T)

    def DetectStereo(self, left: np.ndarray, right: np.ndarray):
        okl, fl = self.Detect(left)
        okr, fr = self.Detect(right)
        ok = okl & okr                                            # feature_detector.cc:74-80
        if not ok:
            print("Failed when extracting point features !")
        return ok, fl, fr


class PointMatcher:
    """Mirror of PointMatcher (include/point_matcher.h:8-24, src/point_matcher.cc).  MatchingPoints' outlier_rejection runs the F-matrix RANSAC
    of :95-104 (cv::findFundamentalMat there) on the device, by the project's contract (include/airfe.h, "F-matrix RANSAC"; not OpenCV's numerics)."""

    def __init__(self, ctx: Context, image_width: int, image_height: int, matcher: int = 0):
        self._ctx = ctx
        self.image_width, self.image_height, self.matcher = image_width, image_height, matcher

    @staticmethod
    def NormalizeKeypoints(features: np.ndarray, width: int, height: int, scale: float) -> np.ndarray:
        """point_matcher.cc:39-48 on a [259, N] matrix."""
        out = np.array(features, dtype=np.float32, order="F", copy=True)
        l_inv = np.float32(1.0 / max(width, height) * float(np.float32(scale)))
        out[1] = (features[1] - np.float32(width // 2)) * l_inv
        out[2] = (features[2] - np.float32(height // 2)) * l_inv
        return out

    def MatchingPoints(self, features0: np.ndarray, features1: np.ndarray, outlier_rejection: bool = False):
        """-> (count, matches) with matches = list of (queryIdx, trainIdx, distance) ≙ cv::DMatch.  outlier_rejection: the reference's fourth argument."""
        if features0.shape[1] < 1 or features1.shape[1] < 1:
            return 0, []                                          # point_matcher.cc:53-55
        scale = 0.7 if self.matcher else 0.5
        n0 = self.NormalizeKeypoints(features0, self.image_width, self.image_height, scale)
        n1 = self.NormalizeKeypoints(features1, self.image_width, self.image_height, scale)
        if self.matcher == 0:
            idx, sc = self._ctx.match_lightglue(np.ascontiguousarray(n0[1:].T), np.ascontiguousarray(n1[1:].T))
            matches = [(int(i), int(j), float(np.float32(1.0) - s)) for (i, j), s in zip(idx, sc)]
        else:
            i0, i1, m0, m1 = self._ctx.match_superglue(np.ascontiguousarray(n0.T), np.ascontiguousarray(n1.T))
            matches = []
            for i in range(len(i0)):                              # point_matcher.cc:82-91
                if 0 <= i0[i] < len(i1) and i1[i0[i]] == i:
                    matches.append((i, int(i0[i]), float(np.float32(1.0 - (m0[i] + m1[i0[i]]) / 2.0))))
        if outlier_rejection and len(matches) > 8:                # point_matcher.cc:95-104
            f0 = np.ascontiguousarray(np.asarray(features0, np.float32).T)
            f1 = np.ascontiguousarray(np.asarray(features1, np.float32).T)
            idx = np.array([(q, t) for q, t, _ in matches], np.int32)
            dist = np.array([d for _, _, d in matches], np.float32)           # carried as the "score": the kernel moves it with its pair, untouched
            kidx, kd = self._ctx.fundamental_ransac(f0, f1, idx, dist)
            matches = [(int(q), int(t), float(d)) for (q, t), d in zip(kidx, kd)]
        return len(matches), matches
