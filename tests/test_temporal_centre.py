"""What pixel-centre guides (pt_render_aovs_centre) do to the preview stack's error on the GPU: the sequences of
tests/temporal_seq.py (128 x 128, 8 frames of 4 spp) rendered through the library with jittered and with centre guides, held to
the numpy restatement's numbers on the CPU reference's frames (python tests/temporal_centre_seq.py)."""
import numpy as np
import pytest

import temporal_ref as T
import temporal_seq as Q
from denoise_ref import mse, passthrough_mask
from test_temporal import _cornell, _report

pytestmark = pytest.mark.gpu

# mse / mse(raw 4 spp) on the last of 8 frames, of the restatement with the library's defaults and CENTRE guides, as
# tests/temporal_centre_seq.py prints them (jittered guides: test_temporal.py's 0.1004 / 0.3136, 0.1357 / 0.2785, 0.4455 / 0.4465).
# The ceiling is that value times 1.05 for the kernel's f32 arithmetic, the margin test_temporal.py grants.
CENTRE_RATIO = {"still": {"var": 0.2078, "hist": 0.1235, "hist_filter": 0.0736},
                "moving": {"var": 0.2106, "hist": 0.2739, "hist_filter": 0.2436}}
# the script's own centre / jittered ratio of history + filter is 0.732 (still) and 0.777 (moving), below the 0.85 at which the
# bound below would have no room
CENTRE_OVER_JITTERED = 0.9


def _sequence(api, gs, moving, centre, links=0, w=Q.W, h=Q.H):
    """test_temporal.py's _sequence with the guide of choice: Q.N_FRAMES frames through the library, the errors of Q.errors."""
    th = api.TemporalHistory(w, h)
    frames = []
    for t in range(Q.N_FRAMES):
        cam = Q.camera(api, t, moving, w, h)
        S, Qs = gs.render_moments(cam, w, h, Q.SPP, Q.SPP // Q.BATCHES, Q.DEPTH, seed=Q.SEED0 + t)
        if centre:
            A, N = gs.render_aovs_centre(cam, w, h, links)
        elif links:
            A, N = gs.render_aovs_chain(cam, w, h, links, aov_spp=1, seed=Q.SEED0 + t)
        else:
            A, N = gs.render_aovs(cam, w, h, aov_spp=1, seed=Q.SEED0 + t)
        hist = th.push(cam, S, Qs, Q.SPP, Q.BATCHES, A, N)
        frames.append((S, Qs, A, N))
    ref, _ = gs.render_moments(cam, w, h, Q.REF_SPP, Q.REF_SPP // 16, Q.DEPTH, seed=Q.REF_SEED)
    filt = api.denoise_hist(hist, A, N)
    m = Q.errors(frames, ref, hist, filt)
    S, Qs, A, N = frames[-1]
    mask = ~passthrough_mask(S, Q.SPP, A) & ~passthrough_mask(ref, Q.REF_SPP, A) & ~T.hist_passthrough(hist)
    m["var_gpu"] = mse(api.denoise_var(S, Qs, Q.SPP, Q.BATCHES, A, N) / Q.SPP, ref / np.float32(Q.REF_SPP), mask)
    m["mean_len"] = float(th.hist_len.mean())
    return m


@pytest.mark.parametrize("name", ["still", "moving"])
def test_quality_centre_guides_beat_jittered_guides(api, gpu_ready, scene_dir, name):
    gs, _ = _cornell(api, scene_dir, "tqc_" + name, Q.W, Q.H, spp=Q.SPP, max_depth=Q.DEPTH)
    moving = name == "moving"
    jit = _sequence(api, gs, moving, False)
    cen = _sequence(api, gs, moving, True)
    _report(name + ", jittered guides", jit)
    _report(name + ", centre guides", cen)
    rc, rj = cen["hist_filter"] / cen["raw"], jit["hist_filter"] / jit["raw"]      # each against its own raw frame, as the script's table
    print("%s: centre / jittered, history + filter: %.3f" % (name, rc / rj))
    want = CENTRE_RATIO[name]
    # 1. the library with centre guides is the restatement with centre guides, within the usual margin
    assert cen["hist"] <= 1.05 * want["hist"] * cen["raw"]
    assert cen["hist_filter"] <= 1.05 * want["hist_filter"] * cen["raw"]
    assert cen["var_gpu"] <= 1.05 * want["var"] * cen["raw"]
    # 2. centre guides beat jittered guides measured here, on the same frames
    assert rc <= CENTRE_OVER_JITTERED * rj
    # 3. with a moving camera the filter no longer loses to the bare history (DESIGN.md §11's inversion)
    if moving:
        assert cen["hist_filter"] <= cen["hist"]


def test_quality_specular_cornell_with_centre_chain_guides_is_reported(api, gpu_ready, scene_dir):
    """test_temporal.py's glass + mirror box with centre guides and a guide chain of 8 next to jittered chain guides. Printed, not
    asserted: nobody has measured it; only that the sequences run and give finite errors."""
    gs, _ = _cornell(api, scene_dir, "tqc_specular", Q.W, Q.H, spp=Q.SPP, max_depth=Q.DEPTH, tall_material=5, short_material=19)
    for moving in (False, True):
        for centre in (False, True):
            m = _sequence(api, gs, moving, centre, links=8)
            _report("specular, %s, %s chain-8 guides" % ("moving" if moving else "still", "centre" if centre else "jittered"), m)
            assert all(np.isfinite(v) for v in m.values())
