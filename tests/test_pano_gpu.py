"""ssfm_pano_synthesize on the GPU against the numpy restatement of the pixel path (tests/_pano_ref.py), evaluated with the job constants of the library's own
plan.  After the plan both sides use only correctly rounded basic operations in the same order, so every comparison is array_equal on the bytes.

Shapes walk the edges of the kernel's tiling: a workgroup is 64 output columns (one wave wide) by 64 rows (four waves, 16 rows each, interleaved), so
pano_width runs through 2, 63, 64, 65, 128, 129, 193, the height through 1, 3, 4, 5 (the waves of a tile), 37, 63, 64, 65, 70, and the frame width through 1 and 48
(a one-pixel frame: every second tap is outside)."""
import functools

import numpy as np
import pytest

from spherical_sfm_amd import _lib, pano

import _pano_ref as PR

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _scene(name, height=None, width=None, pano_width=None):
    s = {"scene1": PR.scene1, "scene2": PR.scene2, "scene3-yaw": lambda: PR.scene3("yaw"), "scene3-pitch": lambda: PR.scene3("pitch")}[name]()
    if height is not None:
        s["height"] = height
    if width is not None:
        s["width"] = width
    if pano_width is not None:
        s["pano_width"] = pano_width
    s["frames"] = PR.texture(len(s["R"]), s["height"], s["width"], seed=7)
    return s


@functools.lru_cache(maxsize=None)
def _flows(kind):
    s = _scene("scene1"); n = len(s["R"])
    if kind == "small":
        return PR.smooth_flows(n, s["height"], s["width"], seed=11, scale=3.0)
    fwd, bwd = PR.smooth_flows(n, s["height"], s["width"], seed=12, scale=25.0 if kind == "large" else 3.0)
    if kind == "nonfinite":
        fwd = fwd.copy(); bwd = bwd.copy()
        fwd[:, 10:20, 15:30, 0] = np.nan; bwd[:, 20:30, 10:25, 1] = np.inf; bwd[2, 3, 4, 0] = -np.inf
    return fwd, bwd


def _check(ctx, s, flows=None, frames=None, **opts):
    frames = s["frames"] if frames is None else frames
    got, owner = pano.synthesize(ctx, s["R"], s["t"], s["intr"], frames, flows, pano_width=s["pano_width"], return_owner=True, **opts)
    popts = {k: v for k, v in opts.items() if k in ("num_phi", "is_loop", "phi_step_deg", "depth", "synth_radius", "synth_focal_factor")}
    P = pano.plan(s["R"], s["t"], s["intr"], s["width"], s["height"], s["pano_width"], **popts)
    stats = {}
    ref, ref_owner = PR.synthesize(P, s["R"], s["t"], s["intr"], frames, flows, s["pano_width"], num_phi=opts.get("num_phi", 9),
                                   subpixel_bits=opts.get("subpixel_bits", 0), stats=stats)
    assert got.dtype == np.uint8 and got.shape == ref.shape
    assert np.array_equal(owner, P["owner"]) and np.array_equal(owner, ref_owner)
    differ = got != ref
    print(f"pixels {got.size // 3}  owned columns {(owner >= 0).mean():.3f}  differing bytes {int(differ.sum())}  taps inside {stats.get('inside', 0)} outside {stats.get('outside', 0)}")
    assert not differ.any(), (int(differ.sum()), np.argwhere(differ)[:5].tolist())
    return got, owner, stats


@pytest.mark.parametrize("name,opts", [("scene1", {}), ("scene1", {"is_loop": 0}), ("scene1", {"num_phi": 1}), ("scene1", {"num_phi": 1, "is_loop": 0}),
                                       ("scene2", {}), ("scene3-yaw", {}), ("scene3-pitch", {})])
def test_linear_mode_scenes(gpu_ctx, name, opts):
    """Scenes 1-3 of tests/test_pano_cpu.py with smooth random textures, no flows: panoramas and owner map."""
    got, owner, stats = _check(gpu_ctx, _scene(name), **opts)
    assert (owner >= 0).any() and got.any()
    assert not got[np.broadcast_to((owner < 0)[:, None, :, None], got.shape)].any()          # columns nobody owns are black
    assert pano.last_kernel_ms(gpu_ctx) > 0.0


@pytest.mark.parametrize("kind", ["small", "large", "nonfinite"])
def test_flow_mode(gpu_ctx, kind):
    """Smooth flows of a few pixels; flows large enough to push samples out of the frame; a flow field with NaN and infinities in it."""
    s = _scene("scene1")
    got, owner, stats = _check(gpu_ctx, s, flows=_flows(kind))
    if kind == "large":
        assert stats["outside"] >= 1 and stats["inside"] >= 1
    if kind == "nonfinite":
        assert stats["invalid"] >= 1
    linear = pano.synthesize(gpu_ctx, s["R"], s["t"], s["intr"], s["frames"], None, pano_width=s["pano_width"])
    assert not np.array_equal(got, linear)                                   # the flows are read


SHAPES = [(2, 37, 48), (63, 37, 48), (64, 37, 48), (65, 37, 48), (128, 37, 48), (129, 37, 48), (193, 1, 48), (193, 3, 48), (193, 4, 48), (193, 5, 48), (193, 63, 48),
          (193, 64, 48), (193, 65, 48), (193, 70, 48), (193, 37, 1), (65, 70, 1)]


@pytest.mark.parametrize("pano_width,height,width", SHAPES)
def test_shapes_at_the_tile_edges(gpu_ctx, pano_width, height, width):
    s = _scene("scene1", height, width, pano_width)
    _check(gpu_ctx, s)
    fwd, bwd = PR.smooth_flows(len(s["R"]), height, width, seed=13, scale=2.0)
    _check(gpu_ctx, s, flows=(fwd, bwd), num_phi=3)


def test_subpixel_bits_5_rounds_the_coordinates(gpu_ctx):
    s = _scene("scene1")
    for flows in (None, _flows("small")):
        snapped, _, _ = _check(gpu_ctx, s, flows=flows, subpixel_bits=5)
        exact, _, _ = _check(gpu_ctx, s, flows=flows, subpixel_bits=0)
        assert not np.array_equal(snapped, exact)                            # the option is not ignored


def test_slab_independence(gpu_ctx):
    """max_slab_bytes forced down to one pair per slab (seven launches, frames uploaded pair by pair) equals the single-slab call."""
    s = _scene("scene1")
    for flows in (None, _flows("small")):
        one = pano.synthesize(gpu_ctx, s["R"], s["t"], s["intr"], s["frames"], flows, pano_width=s["pano_width"])
        per_pair = pano.synthesize(gpu_ctx, s["R"], s["t"], s["intr"], s["frames"], flows, pano_width=s["pano_width"], max_slab_bytes=1)
        assert np.array_equal(one, per_pair)
        bytes_two = 3 * s["height"] * s["width"] * 3 + 2 * 2 * s["height"] * s["width"] * 8 + 4096            # two pairs: three frames, four flow fields
        two = pano.synthesize(gpu_ctx, s["R"], s["t"], s["intr"], s["frames"], flows, pano_width=s["pano_width"], max_slab_bytes=bytes_two)
        assert np.array_equal(one, two)
    s2 = _scene("scene2")
    _check(gpu_ctx, s2, max_slab_bytes=1)
    _check(gpu_ctx, _scene("scene1"), max_slab_bytes=1, is_loop=0)


def test_device_pointer_mode_equals_host_pointer_mode(gpu_ctx):
    import torch
    s = _scene("scene1"); fwd, bwd = _flows("small")
    dev = torch.device("cuda", 0)
    frames_d = [torch.from_numpy(f).to(dev) for f in s["frames"]]
    fwd_d = [torch.from_numpy(f).to(dev) for f in fwd]; bwd_d = [torch.from_numpy(f).to(dev) for f in bwd]
    for flows_h, flows_d in ((None, None), ((fwd, bwd), (fwd_d, bwd_d))):
        host, owner_h = pano.synthesize(gpu_ctx, s["R"], s["t"], s["intr"], s["frames"], flows_h, pano_width=s["pano_width"], return_owner=True)
        got, owner_d = pano.synthesize(gpu_ctx, s["R"], s["t"], s["intr"], frames_d, flows_d, pano_width=s["pano_width"], return_owner=True)
        assert isinstance(got, torch.Tensor) and got.is_cuda and got.dtype == torch.uint8
        assert np.array_equal(got.cpu().numpy(), host) and np.array_equal(owner_h, owner_d)
        assert pano.last_kernel_ms(gpu_ctx) > 0.0
    # one tensor holding all frames works like a list of tensors
    stacked = torch.from_numpy(s["frames"]).to(dev)
    assert np.array_equal(pano.synthesize(gpu_ctx, s["R"], s["t"], s["intr"], stacked, None, pano_width=s["pano_width"]).cpu().numpy(),
                          pano.synthesize(gpu_ctx, s["R"], s["t"], s["intr"], s["frames"], None, pano_width=s["pano_width"]))


def test_repeated_calls_are_equal(gpu_ctx):
    s = _scene("scene2"); n = len(s["R"])
    flows = PR.smooth_flows(n, s["height"], s["width"], seed=14, scale=4.0)
    a = pano.synthesize(gpu_ctx, s["R"], s["t"], s["intr"], s["frames"], flows, pano_width=s["pano_width"])
    b = pano.synthesize(gpu_ctx, s["R"], s["t"], s["intr"], s["frames"], flows, pano_width=s["pano_width"])
    assert np.array_equal(a, b)


def test_constant_frames_give_constant_columns(gpu_ctx):
    """Needs no reference: with every frame one colour c and every tap inside the frames, every owned column is exactly c and every other byte is 0.
    24 cameras 15 degrees apart, focal 20 and a synthetic focal factor of 2 keep the whole map inside 48 x 37 frames (asserted on the restatement's tap count);
    the sweep is open, so some columns have no owner."""
    n = 24
    R, t = PR.circle_poses(n, np.random.default_rng(21))
    intr = (20.0, 23.5, 18.0); opts = dict(synth_focal_factor=2.0, is_loop=0)
    P = PR.plan(R, t, intr, 37, 193, **opts)
    stats = {}
    PR.synthesize(P, R, t, intr, np.zeros((n, 37, 48, 3), np.uint8), None, 193, stats=stats, **opts)
    assert stats["outside"] == 0 and stats["inside"] > 0
    for c in ((255, 0, 128), (1, 2, 3), (77, 201, 254)):
        frames = np.broadcast_to(np.array(c, np.uint8), (n, 37, 48, 3)).copy()
        got, owner = pano.synthesize(gpu_ctx, R, t, intr, frames, None, pano_width=193, return_owner=True, **opts)
        assert (owner >= 0).any() and (owner < 0).any()
        want = np.where((owner >= 0)[:, None, :, None], np.array(c, np.uint8)[None, None, None, :], np.uint8(0))
        assert np.array_equal(got, np.broadcast_to(want, got.shape))


def test_identical_images_in_every_frame(gpu_ctx):
    """Left and right image the same: the blend mixes two remaps of one image, whatever alpha is; linear and flow mode against the restatement."""
    s = _scene("scene1")
    same = np.broadcast_to(s["frames"][:1], s["frames"].shape).copy()
    _check(gpu_ctx, s, frames=same)
    _check(gpu_ctx, s, frames=same, flows=_flows("small"))


def _raw(ctx, s, frames_tab, ff, fb, pano_width, **opts):
    import ctypes as C
    o = pano.options(**opts)
    R = np.ascontiguousarray(s["R"], np.float64); t = np.ascontiguousarray(s["t"], np.float64)
    out = np.zeros((max(o.num_phi, 1), s["height"], max(pano_width, 1), 3), np.uint8)
    f, cx, cy = s["intr"]
    return _lib.lib().ssfm_pano_synthesize(ctx._p, C.byref(o), len(R), R.ctypes.data_as(_lib.c_double_p), t.ctypes.data_as(_lib.c_double_p), f, cx, cy,
                                           s["width"], s["height"], frames_tab, ff, fb, pano_width, C.c_void_p(out.ctypes.data), None)


def test_refusals(gpu_ctx):
    """SSFM_ERR_INVALID with ssfm_last_error set, before the device is touched: the context stays usable and the next call is right."""
    import ctypes as C
    s = _scene("scene1"); n = len(s["R"])
    tab = (C.c_void_p * n)(*[f.ctypes.data for f in s["frames"]])
    fwd, bwd = _flows("small")
    ftab = (C.c_void_p * n)(*[f.ctypes.data for f in fwd])
    L = _lib.lib()
    for kw, ff, fb, frames_tab, pw, msg in (({}, ftab, None, tab, 193, "flow_fwd and flow_bwd"), ({}, None, ftab, tab, 193, "flow_fwd and flow_bwd"),
                                            ({}, None, None, (C.c_void_p * n)(*([tab[0]] * 3 + [None] + [tab[0]] * 3)), 193, "frame 3 is null"),
                                            ({}, None, None, None, 193, "frames is null"),
                                            ({}, None, None, tab, 1, "pano_width < 2"), ({"num_phi": 0}, None, None, tab, 193, "num_phi < 1")):
        rc = _raw(gpu_ctx, s, frames_tab, ff, fb, pw, **kw)
        assert rc == -1                                                        # SSFM_ERR_INVALID
        err = L.ssfm_last_error(gpu_ctx._p).decode()
        assert err.startswith("ssfm_pano_synthesize: ") and msg in err, err
    with pytest.raises(_lib.SsfmError, match="num_phi < 1"):
        pano.synthesize(gpu_ctx, s["R"], s["t"], s["intr"], s["frames"], None, pano_width=193, num_phi=0)
    _check(gpu_ctx, s)
