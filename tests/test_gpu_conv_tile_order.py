"""The two tile orders of the persistent conv kernels (csrc/conv_tile_order.h) byte for byte: raster walk with one launch per cout pass (order 0) against the
XCD-blocked walk with the layer's passes in one launch (order 3 = both kernels), through airfe_debug_conv on the smallest shapes that wrap the tile loop, end in
a partial iteration, keep the raster walk (12 workgroups), decode a tile grid that is no power of two, and run more than one pass.  A tile's arithmetic does
not depend on which workgroup computes it in which iteration: every word of the device buffer, border ring and guards included, must be the same."""
import numpy as np
import pytest

from airslam_amd import api
from gpu_common import context, diag

pytestmark = pytest.mark.gpu

# kernel, B, H, W, cin, cout, form, wgs
CASES = [
    ("conv128r", 3, 16, 32, 128, 128, "plain", 8),      # 12 tiles on 8 workgroups: wraps, half a last iteration
    ("conv128r", 3, 16, 32, 128, 128, "plain", 16),     # grid 12: no multiple of 8, the raster walk under either order
    ("conv128r", 5, 64, 64, 128, 256, "plain", 64),     # two passes in one launch, 4-tile blocks, 5 iterations
    ("conv128r", 2, 32, 32, 128, 128, "pooled", 8),
    ("conv64r", 3, 32, 48, 64, 64, "plain", 8),         # 3 tiles per row: the division decode under the blocked walk
    ("conv64r", 3, 32, 48, 64, 64, "plain", 16),
    ("conv64r", 2, 64, 64, 64, 128, "plain", 16),       # two passes, one tile per XCD and iteration
    ("conv64r", 2, 32, 32, 64, 64, "pooled", 8),
    ("conv64r", 2, 32, 32, 64, 64, "fused", 8),         # conv1a -> conv1b: the patch pipeline walks the same order
]
_INPUTS = {}


def _inputs(B, H, W, cin, cout, form):
    key = (B, H, W, cin, cout, form)
    if key not in _INPUTS:
        rng = np.random.default_rng(sum(key[:5]))
        d = dict(w=(rng.normal(size=(cout, cin, 3, 3)) / np.sqrt(9 * cin)).astype(np.float32), b=(rng.normal(size=cout) * 0.1).astype(np.float32))
        if form == "fused":
            d.update(img=(rng.integers(0, 256, size=(B, H, W)) / 255.0).astype(np.float32), w1a=(rng.normal(size=(64, 9)) / np.sqrt(3.0)).astype(np.float32),
                     b1a=(rng.normal(size=64) * 0.5).astype(np.float32))
        else:
            d["x"] = rng.normal(size=(B, cin, H, W)).astype(np.float32)
        _INPUTS[key] = d
    return _INPUTS[key]


@pytest.fixture
def conv_order():
    """sets the process-wide order for one launch; the library's default is back when the test ends"""
    yield api.conv_tile_order
    api.conv_tile_order(-1)


@pytest.mark.parametrize("kernel,B,H,W,cin,cout,form,wgs", CASES, ids=[f"{c[0]}-B{c[1]}-{c[2]}x{c[3]}-{c[4]}to{c[5]}-{c[6]}-wgs{c[7]}" for c in CASES])
def test_orders_are_byte_equal(kernel, B, H, W, cin, cout, form, wgs, conv_order):
    prec = 1
    ctx, _, _ = context("sp", precision=prec)
    inp = _inputs(B, H, W, cin, cout, form)
    out = {}
    for order in (0, 3):
        conv_order(order)
        out[order] = ctx.debug_conv(inp["w"], inp["b"], prec, x=inp.get("x"), img=inp.get("img"), w1a=inp.get("w1a"), b1a=inp.get("b1a"), pool=form != "plain",
                                    out_pad=1, relu=True, wgs=wgs)
    assert api.conv_tile_order(-1) == 3                  # the switch held what the last launch was given
    for order, o in out.items():
        assert (o["guard_lo"] == 0xFFFF).all() and (o["guard_hi"] == 0xFFFF).all(), f"order {order}: a write outside the output buffer"
        assert not (o["raw"][:, 1:-1, 1:-1, :] == 0xFFFF).any(), f"order {order}: interior words never written"
    diff = out[0]["raw"] != out[3]["raw"]
    if diff.any():
        w = np.argwhere(diff)
        diag(f"conv_tile_order_{kernel}_{B}_{H}x{W}_{cout}_{form}_wgs{wgs}", n_diff=int(diff.sum()), total=diff.size, first=w[0].tolist(), last=w[-1].tolist(),
             images=np.unique(w[:, 0]), rows=np.unique(w[:, 1])[:64], cols=np.unique(w[:, 2])[:64], channels=np.unique(w[:, 3])[:64])
    assert not diff.any(), f"{int(diff.sum())} of {diff.size} words differ between the two tile orders, first at {np.argwhere(diff)[0].tolist()}"


def test_switch_refuses_other_values():
    api.conv_tile_order(-1)
    default = api.conv_tile_order(-1)
    with pytest.raises(api.AirfeError):
        api.conv_tile_order(4)
    assert api.conv_tile_order(-1) == default            # untouched by the refused call
