"""Option "moments_fused": pt_render_moments and its _device / _tiles forms in ONE megakernel launch that keeps the squared batch
sums itself (pt_megakernel.h: MOMENTS) against the B-launch form of the same library, in every bit of S and Q. One case per
kernel family that has a fused twin, both integrators, and batch sizes down to 1 (a boundary at every sample: what a wrong count
of landed samples cannot survive); the CPU reference; tiles that change hands in mid-batch; tile lists at a ragged size; the
launches that fall back; a later pt_render; a preview session.

Sizes: the golden scenes (32 x 32: 16 tiles), and 36 x 20 (15 tiles, the last column and row partial: lanes outside the image)."""
import os

import numpy as np
import pytest

from conftest import GOLDEN, golden_scene
from denoise_var_ref import moments_from_partial_sums
from util import assert_bits_equal

pytestmark = pytest.mark.gpu

SPP_C = [(4, 2), (6, 1), (9, 3)]
HBM = {"onchip": 0, "waves_hbm": 2}          # the kernels for scenes in HBM whatever the tile count
SMALL = {"onchip": 0}                        # ... and their 4-wave forms: 16 tiles do not fill the larger kernels


def _host(api, name):
    return api.HostScene(golden_scene(name, "scenes_tex" if name.startswith("textured") else "scenes"))


def _both(api, hs, opts, render, launches):
    """render(scene) -> (S, Q) with the option off and on, on two scenes of the same options. The fused one must have made
    `launches(B)` launches; the results must be equal bit for bit. Returns (S, Q, the fused scene's flags)."""
    ref, fus = api.Scene(hs, options=opts), api.Scene(hs, options=dict(opts, moments_fused=1))
    assert ref.get_option("moments_fused") == 0 and fus.get_option("moments_fused") == 1
    assert ref.last_moments_launches() == -1 and fus.last_moments_launches() == -1
    try:
        S0, Q0 = render(ref)
        S1, Q1 = render(fus)
        B = int(Q0[0, 0, 3])
        assert ref.last_moments_launches() == B and B >= 2, (ref.last_moments_launches(), B)
        assert fus.last_moments_launches() == launches(B), (fus.last_moments_launches(), B, fus.flags())
        assert_bits_equal(S1, S0, "S"); assert_bits_equal(Q1, Q0, "Q")
        assert np.array_equal(S1.view(np.uint32), S0.view(np.uint32)) or np.isnan(S0).any()
        assert ref.queue_stalls() == 0 and fus.queue_stalls() == 0
        return S1, Q1, fus.flags()
    finally:
        ref.close(); fus.close()


def _cornell(api, scene_dir, name, w, h, **kw):
    from cudapathtracer_amd import scenes
    return api.HostScene(scenes.cornell(os.path.join(scene_dir, name), width=w, height=h, spp=4, max_depth=6, name=name, **kw)["config"])


# ---- 1. one case per kernel family --------------------------------------------------------------------------------------------------
# (scene, options, flags the launch must report with integrator 0, ... with integrator 2). The pair form of FLAT is the MIS
# integrator's only: with the naive one the same scenes take the FLAT closest-hit kernels.
FAMILIES = {
    # (the SIMPLE pair kernel's twin is out of the dispatch, DESIGN.md §9a: with integrator 0 this launch renders in batches)
    "pair_simple": ("cornell32", {}, dict(onchip=1, flat=1, flat_pair=1, simple=1), dict(onchip=1, flat=1, flat_pair=0, simple=1)),
    "pair_lean": ("mixed32", {}, dict(onchip=1, flat_pair=1, simple=0, lean=1), dict(onchip=1, flat=1, flat_pair=0, simple=0)),
    "pair_generic": ("metal32", {"lean": 0}, dict(onchip=1, flat_pair=1, simple=0, lean=0), dict(onchip=1, flat=1, flat_pair=0)),
    "flat_simple": ("cornell32", {"flat2": 0}, dict(onchip=1, flat=1, flat_pair=0, simple=1), dict(onchip=1, flat=1, flat_pair=0, simple=1)),
    "flat_generic": ("mixed32", {"flat2": 0}, dict(onchip=1, flat=1, flat_pair=0, simple=0), dict(onchip=1, flat=1, flat_pair=0, simple=0)),
    "flat_leaf_sync": ("textured32", {}, dict(onchip=1, flat=1, flat_pair=0, simple=0, lean=0), dict(onchip=1, flat=1, flat_pair=0, simple=0)),
    "plain_lds": ("mixed32", {"flat": 0}, dict(onchip=1, flat=0, flat_pair=0), dict(onchip=1, flat=0, flat_pair=0)),
    "plain_lds_leaf": ("textured32", {"flat": 0}, dict(onchip=1, flat=0, flat_pair=0), dict(onchip=1, flat=0, flat_pair=0)),
    "hbm_simple": ("cornell32", HBM, dict(onchip=0, hbm_kernel=1, refill=1, simple=1), dict(onchip=0, hbm_kernel=1, refill=1, simple=1)),
    "hbm_lean": ("mixed32", HBM, dict(onchip=0, hbm_kernel=1, refill=1, simple=0, lean=1), dict(onchip=0, hbm_kernel=1, refill=1, lean=1)),
    "hbm_generic": ("metal32", dict(HBM, lean=0), dict(onchip=0, hbm_kernel=1, refill=1, simple=0, lean=0), dict(onchip=0, hbm_kernel=1, refill=1, lean=0)),
    "hbm_generic_leaf": ("textured32", HBM, dict(onchip=0, hbm_kernel=1, refill=1, simple=0, lean=0), dict(onchip=0, hbm_kernel=1, refill=1, lean=0)),
    "small_simple": ("cornell32", SMALL, dict(onchip=0, hbm_kernel=0, refill=1, simple=1), dict(onchip=0, hbm_kernel=0, refill=1, simple=1)),
    "small_lean": ("mixed32", SMALL, dict(onchip=0, hbm_kernel=0, refill=1, simple=0, lean=1), dict(onchip=0, hbm_kernel=0, refill=1, lean=1)),
    "small_generic": ("textured32", SMALL, dict(onchip=0, hbm_kernel=0, refill=1, simple=0, lean=0), dict(onchip=0, hbm_kernel=0, refill=1, lean=0)),
}


def _assert_flags(fl, want, what):
    got = {k: int(fl[k]) for k in want}
    assert got == want, (what, fl)


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_fused_equals_batches_in_every_kernel_family(api, gpu_ready, family):
    name, opts, want0, want2 = FAMILIES[family]
    hs = _host(api, name)
    w, h, depth, cam = hs.info["width"], hs.info["height"], hs.info["max_depth"], hs.camera()
    for integ, want in ((0, want0), (2, want2)):
        for spp, c in SPP_C:
            what = "%s integrator %d spp %d c %d" % (family, integ, spp, c)
            batches = family == "pair_simple" and integ == 0
            S, Q, fl = _both(api, hs, opts, lambda gs: gs.render_moments(cam, w, h, spp, c, depth, integrator=integ), lambda B: B if batches else 1)
            print(what, fl)
            _assert_flags(fl, want, what)
            assert (Q[..., 3] == spp // c).all() and (Q[..., :3] > 0).mean() > 0.05, what


@pytest.mark.parametrize("simple", [1, 0])
def test_fused_equals_batches_with_128_bit_masks_at_a_ragged_size(api, gpu_ready, scene_dir, simple):
    """72 triangles: the FLAT kernels with 128-bit masks (no pair form beyond 64), with the SIMPLE bounce and with the generic one;
    36 x 20: five of the fifteen tiles have lanes outside the image."""
    hs = _cornell(api, scene_dir, "mf_128", 36, 20, extra_boxes=3)
    cam = hs.camera()
    for integ in (0, 2):
        for spp, c in SPP_C:
            S, Q, fl = _both(api, hs, {"simple": simple}, lambda gs: gs.render_moments(cam, 36, 20, spp, c, 6, integrator=integ), lambda B: 1)
            print("128-bit masks, simple %d integrator %d spp %d c %d" % (simple, integ, spp, c), fl)
            _assert_flags(fl, dict(onchip=1, flat=1, flat_pair=0, simple=simple), "128-bit masks")
            assert S.shape == (20, 36, 4) and (Q[..., 3] == spp // c).all()


# ---- 2. against the CPU reference ------------------------------------------------------------------------------------------------
def test_fused_against_the_cpu_reference(api, oracle, gpu_ready):
    cfg = golden_scene("cornell32")
    hs = api.HostScene(cfg)
    w, h, cam = hs.info["width"], hs.info["height"], hs.camera()
    spp, c, depth = 6, 2, 6
    gs = api.Scene(hs, options={"moments_fused": 1, "flat2": 0})            # the FLAT SIMPLE kernel's twin
    S, Q = gs.render_moments(cam, w, h, spp, c, depth)
    assert gs.last_moments_launches() == 1 and gs.flags()["flat"] and gs.flags()["simple"] and not gs.flags()["flat_pair"], gs.flags()
    osc = oracle.OracleScene(cfg)
    sums = [osc.render(spp=j * c, max_depth=depth, integrator=0, threads=16)[0] for j in range(1, spp // c + 1)]
    assert_bits_equal(S, sums[-1], "S vs the CPU reference")
    assert_bits_equal(Q, moments_from_partial_sums(sums), "Q vs the CPU reference")
    gs.close()


# ---- 3. tiles that change hands in mid-batch -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["lds", "hbm"])
def test_fused_with_tiles_handed_over_inside_a_batch(api, gpu_ready, where):
    hs = _host(api, "mixed32")                                              # LDS-resident: the LEAN pair kernel's twin
    w, h, cam = hs.info["width"], hs.info["height"], hs.camera()
    opts = dict(HBM if where == "hbm" else {}, slice_always=1, sched_mask=0, slice_iters=3)
    ref, fus = api.Scene(hs, options=opts), api.Scene(hs, options=dict(opts, moments_fused=1))
    S0, Q0 = ref.render_moments(cam, w, h, 8, 2, 6)
    S1, Q1 = fus.render_moments(cam, w, h, 8, 2, 6)
    n = fus.tile_handovers()
    print("hand-overs of the fused launch (%s): %d" % (where, n), fus.flags())
    assert n > 0 and fus.last_moments_launches() == 1 and ref.last_moments_launches() == 4
    assert fus.flags()["hbm_kernel"] == (where == "hbm") and fus.flags()["time_slices"], fus.flags()
    assert_bits_equal(S1, S0, where + ": S"); assert_bits_equal(Q1, Q0, where + ": Q")
    assert fus.queue_stalls() == 0
    ref.close(); fus.close()


# ---- 4. tile lists, host and device form ---------------------------------------------------------------------------------------------
def test_fused_on_a_tile_list_at_a_ragged_size(api, gpu_ready, scene_dir):
    torch = gpu_ready
    w, h, spp, c, depth = 36, 20, 6, 2, 6
    hs = _cornell(api, scene_dir, "mf_list", w, h)
    cam = hs.camera()
    tx, ty = 5, 3
    out = (0, 7, tx * ty - 1)                                               # the first tile, a middle one and the last (partial) one are left out
    lst = np.array([t for t in range(tx * ty) if t not in out], np.int32)
    for opts in ({"flat2": 0}, HBM):
        S, Q, fl = _both(api, hs, opts, lambda gs: gs.render_moments_tiles(cam, w, h, spp, c, depth, lst), lambda B: 1)
        for t in range(tx * ty):
            y0, x0 = (t // tx) * 8, (t % tx) * 8
            s, q = S[y0:y0 + 8, x0:x0 + 8], Q[y0:y0 + 8, x0:x0 + 8]
            if t in out:
                assert not s.any() and not q[..., :3].any(), (opts, t)
            else:
                assert s[..., :3].any(), (opts, t)
        assert (Q[..., 3] == spp // c).all()
        # the listed tiles are the full frame's
        full = api.Scene(hs, options=dict(opts, moments_fused=1))
        Sf, Qf = full.render_moments(cam, w, h, spp, c, depth)
        assert full.last_moments_launches() == 1
        live = np.zeros((ty, tx), bool); live.ravel()[lst] = True
        m = np.repeat(np.repeat(live, 8, 0), 8, 1)[:h, :w]
        assert_bits_equal(S[m], Sf[m], "listed tiles: S"); assert_bits_equal(Q[m], Qf[m], "listed tiles: Q")
        # an empty list launches nothing
        Se, Qe = full.render_moments_tiles(cam, w, h, spp, c, depth, np.zeros(0, np.int32))
        assert full.last_moments_launches() == 0 and not Se.any() and not Qe[..., :3].any() and (Qe[..., 3] == spp // c).all()
        # the device forms, on a stream
        dI = torch.from_numpy(lst).to("cuda:0")
        dS = torch.full((h, w, 4), 9.0, device="cuda:0"); dQ = torch.full((h, w, 4), 9.0, device="cuda:0")
        st = torch.cuda.Stream()
        full.render_moments_tiles_device(cam, w, h, spp, c, depth, dI.data_ptr(), lst.size, dS.data_ptr(), dQ.data_ptr(), stream=st.cuda_stream)
        assert full.last_moments_launches() == 1
        assert_bits_equal(dS.cpu().numpy(), S, "list, device form: S"); assert_bits_equal(dQ.cpu().numpy(), Q, "list, device form: Q")
        dS.fill_(3.0); dQ.fill_(5.0)
        full.render_moments_device(cam, w, h, spp, c, depth, dS.data_ptr(), dQ.data_ptr(), stream=st.cuda_stream)
        assert full.last_moments_launches() == 1
        assert_bits_equal(dS.cpu().numpy(), Sf, "device form: S"); assert_bits_equal(dQ.cpu().numpy(), Qf, "device form: Q")
        full.close()


# ---- 5. launches without a fused twin render in batches ------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["wavefront", "culling", "plain_loops"])
def test_launches_without_a_twin_fall_back_to_batches(api, gpu_ready, case):
    hs = _host(api, "mixed32")
    w, h, cam = hs.info["width"], hs.info["height"], hs.camera()
    opts = {"wavefront": {}, "culling": dict(HBM, culling=1), "plain_loops": dict(SMALL, refill=0)}[case]

    def render(gs):
        if case == "wavefront":
            gs.set_variant("wavefront")
        return gs.render_moments(cam, w, h, 6, 2, 6)
    S, Q, fl = _both(api, hs, opts, render, lambda B: B)
    if case == "culling":
        assert fl["culling"] and fl["hbm_kernel"], fl
    if case == "plain_loops":
        assert not fl["refill"] and not fl["onchip"], fl
    # ... and they are the default scene's buffers (culling may differ from them by contract, so it is left out)
    if case != "culling":
        gs = api.Scene(hs)
        S0, Q0 = gs.render_moments(cam, w, h, 6, 2, 6)
        gs.close()
        assert_bits_equal(S, S0, case + ": S vs the default kernels"); assert_bits_equal(Q, Q0, case + ": Q vs the default kernels")


# ---- 6. a later pt_render --------------------------------------------------------------------------------------------------------------
def test_pt_render_after_a_fused_call_is_its_golden(api, gpu_ready):
    g = np.load(os.path.join(GOLDEN, "cornell32_mis.npz"))
    hs = api.HostScene(golden_scene(str(g["scene"])))
    w, h, cam = int(g["w"]), int(g["h"]), hs.camera()
    for opts in ({"flat2": 0}, HBM):
        gs = api.Scene(hs, options=dict(opts, moments_fused=1))
        gs.render(cam, w, h, 2, 4, counters=True)
        before = gs.counters()
        gs.render_moments(cam, w, h, 9, 3, 5, seed=77)
        assert gs.last_moments_launches() == 1 and gs.counters() == before
        col, _ = gs.render(cam, w, h, int(g["spp"]), int(g["max_depth"]))
        assert_bits_equal(col, g["colors"], "pt_render after a fused pt_render_moments %s" % (opts,))
        gs.close()


# ---- 7. a preview session on a scene with the option -----------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [1, 2])
def test_session_on_a_fused_scene_equals_the_session_without(api, gpu_ready, scene_dir, scale):
    import temporal_seq as Q
    w, h = 64, 48
    hs = _cornell(api, scene_dir, "mf_pv", w, h, tall_material=19)          # a mirror box: the LEAN pair kernel, which has a twin in the dispatch
    plain, fused = api.Scene(hs), api.Scene(hs, options={"moments_fused": 1})
    kw = dict(spp=4, batches=2, max_depth=4)
    a, b = api.Preview(plain, w, h, **kw).set_converge(100.0, 2), api.Preview(fused, w, h, **kw).set_converge(100.0, 2)
    a.set_scale(scale); b.set_scale(scale)
    cams = [Q.camera(api, t, True, w, h) for t in range(3)]
    cams += [cams[-1]] * 2                                                  # three moving frames, two resting
    live, launches = [], []
    for t, cam in enumerate(cams):
        x, y = a.frame(cam, Q.SEED0 + t).read(), b.frame(cam, Q.SEED0 + t).read()
        what = "scale %d frame %d" % (scale, t)
        assert_bits_equal(y["mean"], x["mean"], what + ": mean"); assert_bits_equal(y["hist"], x["hist"], what + ": hist")
        assert_bits_equal(y["hist_len"], x["hist_len"], what + ": hist_len")
        assert np.array_equal(y["rgba8"], x["rgba8"]), what
        assert a.last_live() == b.last_live(), what
        live.append(b.last_live()[0]); launches.append((plain.last_moments_launches(), fused.last_moments_launches()))
    print("scale %d: live tiles per frame %s, launches (plain, fused) %s" % (scale, live, launches))
    assert all(p == (2 if n else 0) and f == (1 if n else 0) for n, (p, f) in zip(live, launches)), (live, launches)
    assert launches[0] == (2, 1)
    a.close(); b.close(); plain.close(); fused.close()
