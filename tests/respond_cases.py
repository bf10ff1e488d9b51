"""The shared inputs of the responsive-history tests: the Cornell scene of tests/motion_cases.py (glass tall box, mirror short box) at
the sizes the kernels' paths need, three frames of history on the old geometry, then one change (the tall box moves, or the light
quad) and the frame after it. The frames come from a renderer: tests/test_respond.py uses the library's own (pt_render_moments,
pt_render_aovs_centre, pt_render_motion), tests/test_respond_ref_cpu.py the CPU oracle's, which equal them bit for bit, so an input
whose FRAGILE share breaks the cap is found without a GPU.

A case is everything the last frame's accumulation reads: cam, prev_cam, S, Q, A, N, prev_n, hist, ln, motion, cur (the frame's
working pixels by temporal_ref.frame_ev: the `cur` form of the same frame)."""
import numpy as np

import motion_cases as MC
import temporal_ref as T

SPP, BATCHES, DEPTH = 4, 2, 4
SIZES = ((40, 24), (37, 21), (5, 4))       # whole tiles | partial workgroups and partial wave tiles on both axes | smaller than a window
CHANGES = {"box": (48, 72, MC.SHIFT), "light": (20, 24, (0.3, 0.0, 0.0))}
FRAGILE_CAP = 0.005                        # of a frame: the existing temporal tests' cap
MIN_SHORTENED = {(40, 24): 20, (37, 21): 20, (5, 4): 0}     # pixels with lambda < 1 after the change at the defaults: a condition on the input


def cur_of(S, Qs, A):
    _, e, V, skip = T.frame_ev(S, Qs, SPP, BATCHES, A)
    cur = np.concatenate([e, V[..., None]], -1).astype(np.float32)
    cur[skip, 3] = -1
    return cur


class OracleRenderer:
    """Frames by the CPU reference in oracle/."""

    def __init__(self, api, O, hs):
        self.api, self.O, self.hs = api, O, hs
        self.leaf = hs.info["leaf_size"]
        self.old = MC.arrays(hs)
        self.arrays = self.old
        self.scene = MC.oracle_scene(O, self.old, self.leaf)

    def change(self, first, last, shift):
        self.arrays = MC.moved_arrays(self.hs, first, last, shift)
        self.scene = MC.oracle_scene(self.O, self.arrays, self.leaf)

    def moments(self, cam, w, h, seed):
        from denoise_var_ref import moments_from_partial_sums
        cb = np.frombuffer(cam.tobytes(), np.uint8).copy()
        c = SPP // BATCHES
        sums = [self.scene.render(camera=cb, width=w, height=h, spp=(j + 1) * c, max_depth=DEPTH, integrator=0, seed=seed, threads=4)[0]
                for j in range(BATCHES)]
        return sums[-1], moments_from_partial_sums(sums)

    def guides(self, cam, w, h, motion=False):
        import motion_ref as M
        hits, A, N = MC.oracle_centre_hits(self.O, self.scene, cam, w, h)
        if not motion:
            return A, N
        return A, N, M.motion(self.arrays["points"], self.old["points"], self.arrays["mesh"], hits).reshape(h, w, 4)

    def close(self):
        pass


class LibraryRenderer:
    """Frames by the library on the GPU."""

    def __init__(self, api, hs):
        self.api, self.hs = api, hs
        self.scene = api.Scene.from_mesh(hs)

    def change(self, first, last, shift):
        self.scene.update_vertices(MC.moved_arrays(self.hs, first, last, shift)["points"])

    def moments(self, cam, w, h, seed):
        return self.scene.render_moments(cam, w, h, SPP, SPP // BATCHES, DEPTH, seed=seed)

    def guides(self, cam, w, h, motion=False):
        if not motion:
            return self.scene.render_aovs_centre(cam, w, h, 0)
        return self.scene.render_motion(cam, w, h, guides=True)

    def close(self):
        self.scene.close()


FOV = 25.0


def cameras(api, kind, w, h):
    """Four cameras: "identity" the same bytes four times, "pinhole" a drift with some yaw and pitch per frame. The field of view is
    narrow and the cameras are pitched and rolled a little. At frames this small a 60 degree view steps so far per pixel that on the
    floor and the side walls |z_q - z_p| / (depth_tol z_p) of window pairs spreads evenly over 0..2 and beyond, and about 1 % to
    3 % of the pixels have a pair within 1e-3 of the threshold (seen level, rows 10 and 11 below the horizon differ by exactly 0.10):
    FRAGILE by definition, above the cap. At 25 degrees the pairs on one surface stay well below the threshold and those across
    an edge well above it."""
    if kind == "identity":
        return [api.make_camera(True, (0.02, 0.013, 1.0), (2.3, 1.1, 0.7), FOV, w, h) for _ in range(4)]
    return [api.make_camera(True, (0.03 * t, 0.01 * t, 1.0), (2.3 + 0.3 * t, 0.8 * t, 0.7), FOV, w, h) for t in range(4)]


def build(api, make_renderer, w, h, change, kind):
    """Three frames of history on the old geometry through the restatement's base function (both renderers' frames are the same
    bits, so both sides of every test start from the same history), the change, and the fourth frame."""
    cams = cameras(api, kind, w, h)
    r = make_renderer()
    hist = ln = prev_n = prev_cam = None
    for t in range(3):
        S, Qs = r.moments(cams[t], w, h, 20 + t)
        A, N = r.guides(cams[t], w, h)
        hist, ln, _ = T.accumulate(cams[t], prev_cam, S, Qs, SPP, BATCHES, A, N, prev_n, hist, ln, **T.DEFAULTS)
        prev_n, prev_cam = N, cams[t]
    r.change(*CHANGES[change])
    S, Qs = r.moments(cams[3], w, h, 23)
    A, N, mv = r.guides(cams[3], w, h, motion=True)
    r.close()
    return dict(cam=cams[3], prev_cam=prev_cam, S=S, Q=Qs, A=A, N=N, prev_n=prev_n, hist=hist, ln=ln, motion=mv, cur=cur_of(S, Qs, A), w=w, h=h)


def plant_hazards(c):
    """A copy of the case with pixels that must be skipped: a pass-through pixel (coverage 0), a miss pixel (zero normal and coverage)
    in the current frame, and a non-finite e in a non-pass-through pixel of the history. Returns (case, [(y, x), ...])."""
    c = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in c.items()}
    h, w = c["h"], c["w"]
    spots = [(h // 2, w // 2), (h // 2 - 1, w // 3), (h // 3, w // 2 + 1)]
    (y0, x0), (y1, x1), (y2, x2) = spots
    c["A"][y0, x0, 3] = 0
    c["A"][y1, x1] = 0; c["N"][y1, x1] = 0
    assert c["hist"][y2, x2, 3] >= 0
    c["hist"][y2, x2, 0] = np.inf
    c["cur"] = cur_of(c["S"], c["Q"], c["A"])
    return c, spots


def restate(R, c, form="sums", motion=False, **respond):
    """respond_ref on a case: (hist, hist_len, lambda, fragile)."""
    mv = c["motion"] if motion else None
    if form == "sums":
        return R.accumulate(c["cam"], c["prev_cam"], c["S"], c["Q"], SPP, BATCHES, c["A"], c["N"], c["prev_n"], c["hist"], c["ln"], motion=mv,
                            **T.DEFAULTS, **respond)
    return R.accumulate_cur(c["cam"], c["prev_cam"], c["cur"], c["N"], c["prev_n"], c["hist"], c["ln"], motion=mv, **T.DEFAULTS, **respond)


def library(api, c, form="sums", motion=False, scale=True, **respond):
    """pt_temporal_accumulate_respond (host form) on a case: (hist, hist_len, lambda or None)."""
    mv = c["motion"] if motion else None
    hist = dict(camera_prev=c["prev_cam"], prev_normal_depth=c["prev_n"], hist=c["hist"], hist_len=c["ln"], motion=mv, scale=scale)
    if form == "sums":
        return api.temporal_accumulate_respond(c["cam"], c["N"], c["S"], c["Q"], SPP, BATCHES, c["A"], **hist, **respond)
    return api.temporal_accumulate_respond(c["cam"], c["N"], cur=c["cur"], **hist, **respond)
