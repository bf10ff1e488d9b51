"""Analytic frames for the post-process kernels (pt_denoise, pt_denoise_var, pt_denoise_hist, pt_temporal_accumulate*, pt_upsample):
feature buffers of a small world of bounded planes seen by any pt_camera, synthetic moments for them with planted edge pixels, and
the camera pairs that reach each branch of the reprojection. numpy only: nothing here touches a GPU or renders a scene.

tests/test_postfx_cases.py shows without a GPU that the cases mean what they claim; tests/test_postfx_edges.py runs the kernels on
them against the numpy restatements (denoise_ref, denoise_var_ref, temporal_ref, upsample_ref).

The world (units as the Cornell scenes': the camera rests at z = 3 and looks down -z):
  wall    z = 0, |x| <= 8, -1 <= y <= 1.2                       the back wall; above it and past its ends lies empty space
  slab    z = 1, -0.9 <= x <= -0.2, -0.5 <= y <= 0.6            nearer: depth steps, and disocclusion behind it when the camera moves
  floor   y = -1, |x| <= 8, 0 <= z <= 2.5                       its green albedo 0.005 < 0.01: the demodulation fallback a = 1
  tilted  through (0.9, 0, 0.6), turned 37 degrees about y      n . n_wall = cos 37 = 0.799: below a normal_tol of 0.9
Planes are hit from both sides and keep their stated normal. A pixel's ray is the UNJITTERED CENTRE RAY of include/pt_api.h
(pt_temporal_accumulate, step 3): t = right u + up v + forward through pixel x, not x + 0.5. Intersections are float64; the depth
is the distance along the normalised ray; normals are stored with length 0.5, not 1, so a kernel that skips the normalisation shows."""
import numpy as np

import temporal_ref as T
from denoise_var_ref import moments_from_partial_sums

f32 = np.float32
SPP, BATCHES = 4, 2
FOV = 60.0
NORMAL_LEN = 0.5
TILT = np.radians(37.0)


def _patch(name, origin, normal, a, b, a_lim, b_lim, albedo):
    return {"name": name, "o": np.array(origin, np.float64), "n": np.array(normal, np.float64), "a": np.array(a, np.float64),
            "b": np.array(b, np.float64), "a_lim": a_lim, "b_lim": b_lim, "albedo": albedo}


WORLD = (
    _patch("wall", (0, 0, 0), (0, 0, 1), (1, 0, 0), (0, 1, 0), (-8.0, 8.0), (-1.0, 1.2), (0.7, 0.7, 0.7)),
    _patch("slab", (0, 0, 1), (0, 0, 1), (1, 0, 0), (0, 1, 0), (-0.9, -0.2), (-0.5, 0.6), (0.8, 0.3, 0.2)),
    _patch("floor", (0, -1, 0), (0, 1, 0), (1, 0, 0), (0, 0, 1), (-8.0, 8.0), (0.0, 2.5), (0.6, 0.005, 0.4)),
    _patch("tilted", (0.9, 0, 0.6), (np.sin(TILT), 0, np.cos(TILT)), (np.cos(TILT), 0, -np.sin(TILT)), (0, 1, 0), (-0.5, 0.5), (-0.6, 0.7),
           (0.2, 0.5, 0.8)),
)
SURFACE = {p["name"]: i for i, p in enumerate(WORLD)}
MISS = -1


def centre_rays(cam):
    """(origin [3], unit directions [h,w,3]) of the camera's unjittered centre rays, float64 from the camera's float32 fields."""
    c = T.camera_fields(cam)
    w, h = c["w"], c["h"]
    ys, xs = np.mgrid[0:h, 0:w]
    fov = float(c["fovScale"])
    u = (2.0 * (xs / w) - 1.0) * (float(f32(w) / f32(h))) * fov
    v = (2.0 * (ys / h) - 1.0) * fov
    t = (c["right"].astype(np.float64) * u[..., None] + c["up"].astype(np.float64) * v[..., None]) + c["forward"].astype(np.float64)
    return c["origin"].astype(np.float64), t / np.linalg.norm(t, axis=-1, keepdims=True)


def trace(cam):
    """The nearest patch along every centre ray: (surface index [h,w], MISS where nothing is hit; distance [h,w] float64)."""
    o, d = centre_rays(cam)
    best = np.full(d.shape[:2], np.inf)
    which = np.full(d.shape[:2], MISS)
    for i, p in enumerate(WORLD):
        dn = d @ p["n"]
        with np.errstate(divide="ignore", invalid="ignore"):
            t = ((p["o"] - o) @ p["n"]) / dn
            P = o + t[..., None] * d - p["o"]
            la, lb = P @ p["a"], P @ p["b"]
        hit = (dn != 0) & (t > 1e-9) & (la >= p["a_lim"][0]) & (la <= p["a_lim"][1]) & (lb >= p["b_lim"][0]) & (lb <= p["b_lim"][1]) & (t < best)
        best = np.where(hit, t, best)
        which = np.where(hit, i, which)
    return which, best


def guides(cam):
    """(albedo, normal_depth) [h,w,4] float32 as pt_render_aovs lays them out: albedo.w is the coverage (1 hit, 0 miss), the normal
    has length NORMAL_LEN, normal_depth.w is the distance along the centre ray; a miss is all zeros."""
    which, t = trace(cam)
    A = np.zeros(which.shape + (4,), f32); N = np.zeros(which.shape + (4,), f32)
    for i, p in enumerate(WORLD):
        m = which == i
        A[m, :3] = p["albedo"]; A[m, 3] = 1.0
        N[m, :3] = NORMAL_LEN * p["n"]; N[m, 3] = t[m]
    return A, N


# ---- moments -----------------------------------------------------------------------------------------------------------------------
EDGE_KINDS = ("s_nan", "s_inf", "q_nan", "zero_normal", "v_zero")


def edge_places(albedo):
    """Five distinct hit pixels spread over the frame, one per kind of EDGE_KINDS; {} for a frame with fewer than ten hit pixels."""
    ys, xs = np.nonzero(albedo[..., 3] > 0)
    if ys.size < 10:
        return {}
    k = (np.arange(1, 6) * ys.size) // 6
    return {kind: (int(ys[i]), int(xs[i])) for kind, i in zip(EDGE_KINDS, k)}


def moments(albedo, normal_depth, seed, plant=None, level=1.0):
    """(S, Q, albedo, normal_depth) of SPP samples in BATCHES batches for the given guides: every batch adds albedo * level * u,
    u uniform in [0.2, 1) per pixel and channel, so e is about 0.6 level on every surface (level: a number or [h,w]); S and Q are 0
    where the coverage is 0. Q
    is moments_from_partial_sums of the batches. plant: {kind: (y, x)} of EDGE_KINDS; the guides come back as copies (the zero
    normal is planted in normal_depth). v_zero: both batches add the same powers of two, so Q = S S / B exactly and V = 0."""
    rng = np.random.default_rng(seed)
    A = np.array(albedo, f32); N = np.array(normal_depth, f32)
    h, w = A.shape[:2]
    plant = plant or {}
    hit = (A[..., 3] > 0)[..., None]
    level = np.broadcast_to(np.asarray(level, f32), (h, w))[..., None]
    acc = np.zeros((h, w, 4), f32); partial = []
    for _ in range(BATCHES):
        acc = acc.copy()
        add = (A[..., :3] * level * rng.uniform(0.2, 1.0, (h, w, 3)).astype(f32)).astype(f32) * f32(SPP // BATCHES)
        if "v_zero" in plant:
            add[plant["v_zero"]] = (0.5, 0.25, 0.125)
        acc[..., :3] = (acc[..., :3] + np.where(hit, add, f32(0))).astype(f32)
        partial.append(acc)
    S, Q = partial[-1].copy(), moments_from_partial_sums(partial)
    if "s_nan" in plant:
        S[plant["s_nan"]][0] = np.nan
    if "s_inf" in plant:
        S[plant["s_inf"]][1] = np.inf
    if "q_nan" in plant:
        Q[plant["q_nan"]][2] = np.nan
    if "zero_normal" in plant:
        N[plant["zero_normal"]][:3] = 0.0
    return S, Q, A, N


def frame(cam, seed, plant=False, level=1.0):
    """guides(cam) and their moments; plant=True plants edge_places."""
    A, N = guides(cam)
    return moments(A, N, seed, edge_places(A) if plant else None, level)


# ---- cameras -------------------------------------------------------------------------------------------------------------------------
HOME = (0.0, 0.0, 3.0)
FILTER_POSE = ((-0.2, 0.1, 3.0), (0.0, -15.0, 180.0))   # rolled: the floor fills the last rows, empty space the first
SIDEWAYS = 0.03                           # world units: 0.37 of a pixel on the wall at 61 x 43, less at every smaller size


def camera(api, w, h, pos=HOME, rot=(0.0, 0.0, 0.0)):
    return api.make_camera(True, pos, rot, FOV, w, h)


def filter_camera(api, w, h):
    """The filters' yawed and rolled view: every surface and empty space are in a frame as wide as 17 x 9 or
    61 x 43. A frame of one pixel stays upright: its only ray is the frame's corner ray, which the rolled view sends into empty space."""
    pos, rot = FILTER_POSE
    return camera(api, w, h, pos, rot if w * h > 1 else (rot[0], rot[1], 0.0))


PAIRS = ("same", "sideways", "yaw25", "yaw70", "behind", "about_face")


def camera_pair(api, name, w, h):
    """(previous, current) camera of a temporal case, positions and angles in world units and degrees."""
    home = camera(api, w, h)
    if name == "same":                    # the same bytes: the identity path
        return api.Camera.frombytes(home.tobytes()), home
    if name == "sideways":                # a fraction of a pixel to the right: every projection moves, the last column's leaves [0, w - 1]
        return home, camera(api, w, h, (SIDEWAYS, 0.0, 3.0))
    if name == "yaw25":                   # a turn of a third of the view and a small move
        return home, camera(api, w, h, (-0.4, 0.05, 2.9), (0.0, 25.0, 0.0))
    if name == "yaw70":                   # the current camera looks past the wall's end into empty space
        return home, camera(api, w, h, HOME, (0.0, 70.0, 0.0))
    if name == "behind":                  # previous close to the wall, current far back and pitched down: much of what it sees lay behind
        # the previous camera. At z = 0.5 it stands midway between the wall and the slab: a slab point mirrored through the camera
        # lands on the wall at the slab point's own distance and with its normal, so only the z_c > 0 test keeps that tap out
        return camera(api, w, h, (0.0, 0.0, 0.5)), camera(api, w, h, (0.0, 0.8, 4.5), (-15.0, 0.0, 0.0))
    if name == "about_face":              # nothing lies behind home
        return home, camera(api, w, h, HOME, (0.0, 180.0, 0.0))
    raise KeyError(name)


HIST_LEN_SCALE = 7.0                      # the history's lengths are multiplied by this: N_h + 1 = 8 > OFF_DEFAULT's max_history
OFF_DEFAULT = {"max_history": 5, "depth_tol": 0.03, "normal_tol": 0.97}


def temporal_case(api, name, w, h):
    """Everything a temporal case feeds pt_temporal_accumulate, made without a GPU: the two cameras, the current frame (S, Q, A, N) with
    planted edge pixels, the previous guide and the previous history. The history is the restatement's first frame of the previous
    camera (the frame's own e and V: no arithmetic of the blend), its lengths times HIST_LEN_SCALE, and one planted pass-through pixel
    that holds NaN."""
    prev, cur = camera_pair(api, name, w, h)
    f0 = frame(prev, 100)
    f1 = frame(cur, 101, plant=True)
    hist, ln, _ = T.accumulate(prev, None, f0[0], f0[1], SPP, BATCHES, f0[2], f0[3])
    ln = (ln * f32(HIST_LEN_SCALE)).astype(f32)
    ys, xs = np.nonzero(hist[..., 3] >= 0)
    planted = None
    if ys.size >= 3:
        planted = (int(ys[ys.size // 2]), int(xs[ys.size // 2]))
        hist[planted] = (np.nan, np.nan, np.nan, -1.0); ln[planted] = 0
    return {"name": name, "w": w, "h": h, "prev": prev, "cur": cur, "frame": f1, "prev_nd": f0[3], "hist": hist, "hist_len": ln, "planted": planted}


def restate_temporal(case, **params):
    """temporal_ref.accumulate on a case: (hist, hist_len, fragile)."""
    S, Q, A, N = case["frame"]
    return T.accumulate(case["cur"], case["prev"], S, Q, SPP, BATCHES, A, N, case["prev_nd"], case["hist"], case["hist_len"], **params)


def branch_counts(case, out_len, params):
    """How many pixels of a case take each branch of step 3 and 4, from the restatement alone. Over the pixels that blend at all (not
    pass-through, a nonzero normal): behind (z_c <= 0), off_screen, edge_tap (x' in [-1, 0) or [w - 1, w), or y' likewise: a row or
    column of taps lies outside; edge_low and edge_high say on which side), inside; found = the pixels that took history, clamped = those whose length max_history decided."""
    S, Q, A, N = case["frame"]
    w, h = case["w"], case["h"]
    skip = T.frame_ev(S, Q, SPP, BATCHES, A)[3]
    blend = ~skip & ~T.unit_normals(N)[1]
    identity = T.camera_fields(case["prev"])["bytes"] == T.camera_fields(case["cur"])["bytes"]
    xp, yp, _, front = T.reproject(case["cur"], case["prev"], N[..., 3])
    with np.errstate(invalid="ignore"):
        on = front & (xp >= -1) & (xp < w) & (yp >= -1) & (yp < h)
        low, high = on & ((xp < 0) | (yp < 0)), on & ((xp >= w - 1) | (yp >= h - 1))
        edge = low | high
    found = ~skip & (out_len > 1)
    return {"pixels": int(skip.size), "pass_through": int(skip.sum()), "blend": int(blend.sum()), "identity": bool(identity),
            "behind": int((blend & ~front).sum()), "off_screen": int((blend & front & ~on).sum()),
            "edge_tap": 0 if identity else int((blend & edge).sum()), "edge_low": 0 if identity else int((blend & low).sum()),
            "edge_high": 0 if identity else int((blend & high).sum()), "inside": int((blend & on & ~edge).sum()),
            "found": int(found.sum()), "found_share": float(found.sum()) / max(1, int((~skip).sum())),
            "clamped": int((found & (out_len == f32(params["max_history"]))).sum())}


def check_branches(case, counts, params):
    """What each pair must produce (the table of DESIGN.md's testing notes). The branch counts hold at every size a pair is run at;
    the shares of found history are properties of the 61 x 43 view (7 x 19 is a slit 24 degrees wide, 17 x 9 spans 95 degrees), and
    edge taps next to off-screen pixels need a frame that keeps part of the previous view (17 x 9 and 61 x 43)."""
    name, w, h = case["name"], case["w"], case["h"]
    full = (w, h) == (61, 43)
    what = "%s %d x %d: %s" % (name, w, h, counts)
    if name == "same":
        assert counts["identity"] and counts["found"] > 0, what
    if name == "sideways":
        assert not counts["identity"] and counts["edge_high"] >= 1 and counts["found"] > 0, what
        assert not full or counts["found_share"] > 0.9, what
    if name == "yaw25":
        assert counts["off_screen"] > 0 and (w < 17 or counts["edge_low"] > 0), what
        assert not full or 0.3 < counts["found_share"] < 0.7, what
    if name == "yaw70":
        assert counts["pass_through"] > 0 and counts["off_screen"] > 0, what
        assert not full or counts["found_share"] < 0.5, what
    if name == "behind":
        assert counts["behind"] > 0, what
    if name == "about_face":
        assert counts["pass_through"] == counts["pixels"] and counts["found"] == 0, what
    if counts["found"] and params["max_history"] < HIST_LEN_SCALE + 1:
        assert counts["clamped"] >= 1, what


# ---- every dispatch target of pt_temporal.hip at a ragged size -------------------------------------------------------------------
RAGGED = (17, 9)                          # two workgroups in x; 3 x 2 tiles, the last column one pixel wide and the last row one pixel high
RAGGED_PAIRS = ("same", "sideways")       # the identity and the projecting instantiations
RAGGED_LIVE = np.array([[1, 0, 1], [0, 1, 0]], np.int32)      # live and carried tiles, of both a partial one


def ragged_case(api, name):
    """temporal_case at RAGGED with what the other entry points need: `working`, the frame's (e, V) as pt_temporal_accumulate_cur
    takes them, one hit pixel's variance NaN (it passes through there, and nowhere else); `motion`, a synthetic motion buffer: every
    third pixel that has a right neighbour has w = 1 and the world point of that neighbour's guide as xyz, all others are 0."""
    w, h = RAGGED
    case = temporal_case(api, name, w, h)
    S, Q, A, N = case["frame"]
    m, e, V, skip = T.frame_ev(S, Q, SPP, BATCHES, A)
    cur = np.concatenate([np.where(skip[..., None], m, e), np.where(skip, f32(-1), V)[..., None]], -1).astype(f32)
    ys, xs = np.nonzero(~skip)
    cur[ys[ys.size // 3], xs[ys.size // 3], 3] = np.nan
    o, d = centre_rays(case["cur"])
    P = o + d * N[..., 3:4].astype(np.float64)
    idx = np.arange(h * w).reshape(h, w)
    moved = (idx % 3 == 1) & (idx % w < w - 1)
    motion = np.zeros((h, w, 4), f32)
    motion[moved, :3] = np.roll(P, -1, axis=1)[moved]
    motion[moved, 3] = 1
    return dict(case, working=cur, motion=motion)


def check_ragged_case(case, motion_len):
    """What the restatement's result with the motion buffer (its lengths) and the map must show, so that the kernels' agreement
    with it says something: moved pixels that found history and one that did not, partial tiles of both kinds, a pass-through pixel
    in a live tile."""
    w, h = RAGGED
    moved = case["motion"][..., 3] == 1
    assert (moved & (motion_len > 1)).sum() >= 4 and (moved & (motion_len == 1)).sum() >= 1
    ty, tx = RAGGED_LIVE.shape
    assert (ty, tx) == ((h + 7) // 8, (w + 7) // 8) and (w % 8 or h % 8)
    partial = np.zeros((ty, tx), bool)
    if w % 8: partial[:, -1] = True
    if h % 8: partial[-1, :] = True
    assert (partial & (RAGGED_LIVE != 0)).any() and (partial & (RAGGED_LIVE == 0)).any()
    live = np.repeat(np.repeat(RAGGED_LIVE != 0, 8, axis=0), 8, axis=1)[:h, :w]
    assert ((motion_len == 0) & live).any()


# ---- upsample ------------------------------------------------------------------------------------------------------------------------
UPSAMPLE_SHAPES = ((1, 1, 8), (2, 3, 8), (7, 5, 5))          # (wl, hl, s)


def upsample_case(api, wl, hl, s, yawed):
    """(S, Q, albedo_lo, normal_depth_lo, albedo, normal_depth): a low-res frame of scaled_camera(cam, s), with planted edge pixels
    where it has ten hit pixels, and the display guides of cam."""
    w, h = wl * s, hl * s
    cam = camera(api, w, h, FILTER_POSE[0], (0.0, FILTER_POSE[1][1], 0.0)) if yawed else camera(api, w, h)     # (upright: low-res pixel 0 must hit)
    lo = frame(api.scaled_camera(cam, s), 200 + s, plant=True)
    A, N = guides(cam)
    return lo + (A, N)


# ---- filters -------------------------------------------------------------------------------------------------------------------------
# 1 x 1; 7 x 19: narrower than one 8 x 8 wave tile, three workgroup rows; 17 x 9: one pixel over a 16 x 16 workgroup and over a tile in
# both axes, less than one block of 256 pixels; 61 x 43; 300 x 221: 259 partial sums, so the reduction's strided loop runs a second
# round, and the last block of the prepare and finish kernels holds 252 pixels.
FILTER_SIZES = ((1, 1), (7, 19), (17, 9), (61, 43), (300, 221))
TEMPORAL_SIZES = ((7, 19), (17, 9), (61, 43))
# None: the library's default count. 16 is the largest count the library takes (a step of 32 768: every tap lies outside the image).
ITERATIONS = {(1, 1): (0, 1, None), (7, 19): (0, 1, None), (17, 9): (0, 1, 16, None), (61, 43): (0, 1, 16, None), (300, 221): (0, 1, 2)}
DENOISE_OFF = {"iterations": 2, "sigma_color": 2.0, "sigma_normal": 0.0, "sigma_depth": 0.04}
VAR_OFF = {"iterations": 2, "sigma_var": 2.0, "sigma_normal": 0.0, "sigma_depth": 0.04}


REDUCE_ROUND = 256 * 256                  # pixels whose partial sums one round of denoise_reduce_kernel's loop covers: 256 threads, 256 pixels each
TAIL_LEVEL = 200.0


def filter_frame(api, w, h):
    """(S, Q, A, N) of the filters' yawed view with planted edge pixels. The pixels from REDUCE_ROUND on, whose partial sums the
    reduction meets in its second round (300 x 221 has 764 of them, floor and wall), are TAIL_LEVEL times brighter: they carry two
    thirds of the frame's luminance, so an L that leaves them out is a third of the right one and moves every weight."""
    level = np.where(np.arange(h * w).reshape(h, w) >= REDUCE_ROUND, f32(TAIL_LEVEL), f32(1))
    return frame(filter_camera(api, w, h), 300, plant=True, level=level)


def history_of(S, Q, A, N):
    """A frame as a history buffer (pt_denoise_hist's input): the restatement's first frame, the frame's own (e, V)."""
    return T.accumulate(None, None, S, Q, SPP, BATCHES, A, N)[0]


def pass_through_frame(w, h, seed=301):
    """Nothing is hit: coverage 0 everywhere over sums that are not 0, so every pixel passes through and no pixel counts towards L."""
    rng = np.random.default_rng(seed)
    S = rng.uniform(0.1, 2.0, (h, w, 4)).astype(f32)
    Q = rng.uniform(0.1, 2.0, (h, w, 4)).astype(f32); Q[..., 3] = BATCHES
    return S, Q, np.zeros((h, w, 4), f32), np.zeros((h, w, 4), f32)


def black_frame(api, w, h):
    """The filters' view with no light in it: every hit pixel is filtered, e = 0, V = 0 and L = 0."""
    A, N = guides(filter_camera(api, w, h))
    Q = np.zeros(A.shape, f32); Q[..., 3] = BATCHES
    return np.zeros(A.shape, f32), Q, A, N


def exchanges(params, keys):
    """params with the values of every two of `keys` exchanged: (key, key, dict)."""
    for i, a in enumerate(keys):
        for b in keys[i + 1:]:
            q = dict(params); q[a], q[b] = params[b], params[a]
            yield a, b, q


def assert_exchanges_matter(restate, params, keys, what):
    """restate(**params) -> (values, compared mask, atol). Exchanging any two of the parameters must move the restatement by more than
    the comparison's tolerance on some compared pixel (a NaN counts): a launch site that passes two of them in the wrong order shows."""
    base, use, atol = restate(**params)
    for a, b, q in exchanges(params, keys):
        with np.errstate(all="ignore"):
            other = restate(**q)[0]
        close = np.isclose(other[use], base[use], rtol=1e-3, atol=atol)
        assert not close.all(), "%s: exchanging %s and %s leaves the restatement within the tolerance" % (what, a, b)
