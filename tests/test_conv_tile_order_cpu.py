"""csrc/conv_tile_order.h on the host: tools/conv_tile_order_check.cpp enumerates the (workgroup, iteration) -> (pass, image, tile) map of the persistent conv
kernels for both orders — the benchmark's shapes at 128 images and 256 workgroups, small batches with wrapped loops and partial last iterations, the grids that
keep the raster walk (12 workgroups, passes that do not divide grid / 8), a tile grid that is no power of two, 1 / 2 / 4 cout passes — and asserts: every
(pass, tile) exactly once, tiles per workgroup within one of each other, the passes of a tile on one XCD in one iteration, an XCD's tiles of one iteration one
compact rectangle of one image (or whole images), and the share of halo neighbours that meet on one XCD in one iteration no lower than the raster order's.
Built as a stand-alone program with the address and undefined-behaviour sanitizers; nothing is loaded into this process."""
import os
import re
import subprocess

from conftest import ROOT

CSRC = os.path.join(ROOT, "airslam_amd", "csrc")


def test_tile_order_map(tmp_path):
    exe = str(tmp_path / "conv_tile_order_check")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + CSRC,
                        os.path.join(ROOT, "tools", "conv_tile_order_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("ok") and not r.stderr, (r.stdout[-3000:], r.stderr[-3000:])
    share = {m[1].strip(): (int(m[2]), float(m[3]), float(m[4]))
             for m in re.finditer(r"^(.+?) passes (\d): .*raster ([\d.]+), blocked ([\d.]+)$", r.stdout, flags=re.M)}
    # the raster walk at 256 workgroups, read off the kernels: lower neighbour on the same XCD in the same iteration except at a wrap (conv64r 512 x 512:
    # 7 of 8 rows), right neighbour never; 64 x 64: neither
    assert share["conv1 fused 512x512"][1] < 0.5 and share["conv2a/2b 256x256"][1] == 0.5 and share["conv4a/4b 64x64"][1] == 0.0
    for name in ("conv1 fused 512x512", "conv2a/2b 256x256", "conv3a 128x128 64->128", "conv3b/line 128x128"):
        assert share[name][2] > 0.8 > share[name][1], (name, share[name])
    assert share["conv4a/4b 64x64"][2] == 1.0                       # one image per XCD and iteration
    assert share["convPa/Da 64x64 128->256"][2] == round(48 / 52, 4)   # two passes: 16 tiles = half an image, 48 of its 52 neighbour pairs
