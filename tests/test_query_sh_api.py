"""SH queries without a GPU: the new symbols of the C ABI and of the Python wrapper, pt_query_sh_workspace_bytes, every argument check
of pt_query_sh and pt_query_sh_rays_device in the header's order (they fire before any HIP call, under the function's name; n == 0
returns 0 before the scene or anything else is looked at), the record builders and the SH helpers of cudapathtracer_amd/rays.py
against quadrature, the host restatement's map and tree, and the resources of the six sh kernels read from the code-object notes
against DESIGN.md §27's table."""
import os
import sys

import numpy as np
import pytest

import sh_ref as SR

N = 5
WALK, RAYS = "pt_query_sh", "pt_query_sh_rays_device"


def _err(api):
    return api.lib().pt_last_error().decode()


def test_new_symbols_are_declared_and_exported(api):
    from conftest import ROOT
    L = api.lib()
    header = open(os.path.join(ROOT, "include", "pt_api.h")).read()
    for n in ("pt_query_sh_workspace_bytes", "pt_query_sh_device", "pt_query_sh", "pt_query_sh_rays_device"):
        assert hasattr(L, n), n
        assert n + "(" in header, n
    assert hasattr(api.Scene, "query_sh") and hasattr(api.Scene, "query_sh_rays")
    from cudapathtracer_amd import rays
    for n in ("sh_records", "sh_grid", "sh_basis", "sh_irradiance"):
        assert hasattr(rays, n), n


def test_workspace_bytes(api):
    L = api.lib()
    assert L.pt_query_sh_workspace_bytes(7, 1) == 0 and L.pt_query_sh_workspace_bytes(7, 64) == 0
    assert L.pt_query_sh_workspace_bytes(7, 128) == 7 * 2 * 9 * 16
    assert L.pt_query_sh_workspace_bytes(7, 4096) == 7 * 64 * 9 * 16
    assert L.pt_query_sh_workspace_bytes(1 << 16, 4096) == (1 << 22) * 9 * 16              # the largest launch: past 2^29 bytes
    assert L.pt_query_sh_workspace_bytes(0, 4096) == 0


def _buffers():
    recs = np.zeros((N, 8), np.float32)
    out = np.full((N * 64, 8), 77.0, np.float32)               # holds N * 9 float4, and N * 64 rays
    work = np.full((N * 2 * 9, 4), 78.0, np.float32)
    fake = np.zeros(4096, np.uint8)                            # stands for a scene where a check before the scene's must fire
    return recs, out, work, fake


def test_sh_argument_checks_in_order(api):
    """Each case breaks one argument, alone and then together with arguments that later checks of the header's list refuse (`also`):
    the earliest broken check answers, so the message shows the order. The host form has no workspace argument."""
    L = api.lib()
    recs, out, work, fake = _buffers()
    r, o, w, s = recs.ctypes.data, out.ctypes.data, work.ctypes.data, fake.ctypes.data
    good = dict(scene=s, n=N, recs=r, lanes=4, spp_lane=2, max_depth=8, integrator=0, use_mis=1, seed=1, first_stream=0, out=o, work=w, flags=0)
    far = 0xffffffff
    cases = [
        # 1. n < 0 or n * L > 1 << 28
        (dict(n=-1), dict(scene=None, lanes=3, spp_lane=0, integrator=1, flags=4, first_stream=far, work=None), "n -1 at"),
        (dict(n=(1 << 26) + 1), dict(recs=None, spp_lane=0, integrator=1, flags=1), "n 67108865 at 4 lanes must be 0..268435456"),
        (dict(n=(1 << 16) + 1, lanes=4096), dict(out=None, integrator=3, work=None), "n 65537 at 4096 lanes must be"),
        # 2. a NULL scene, records or coefficient buffer
        (dict(scene=None), dict(lanes=3, spp_lane=0, integrator=1, flags=4, first_stream=far, work=None), "null scene"),
        (dict(recs=None), dict(lanes=0, spp_lane=0, integrator=1, flags=4, first_stream=far), "null records"),
        (dict(out=None), dict(lanes=8192, spp_lane=0, integrator=1, flags=1, first_stream=far, work=None), "null output buffer"),
        # 3. lanes
        (dict(lanes=0), dict(spp_lane=0, integrator=1, flags=4, first_stream=far), "lanes 0 must be a power of two in 1..4096"),
        (dict(lanes=3), dict(spp_lane=0, integrator=1, flags=4, first_stream=far), "lanes 3 must be"),
        (dict(lanes=8192), dict(spp_lane=-1, integrator=1, flags=1, work=None), "lanes 8192 must be"),
        (dict(lanes=192), dict(spp_lane=-1, work=None), "lanes 192 must be"),
        (dict(lanes=-4), dict(integrator=1, flags=4), "lanes -4 must be"),
        # 4. spp_lane < 1 or L * spp_lane > 1 << 22
        (dict(spp_lane=0), dict(integrator=1, flags=4, first_stream=far), "spp_lane 0 at 4 lanes must be 1..4194304"),
        (dict(spp_lane=-2, lanes=1), dict(integrator=1, flags=4, first_stream=far), "spp_lane -2 at 1 lanes"),
        (dict(spp_lane=(1 << 20) + 1), dict(integrator=3, flags=1), "spp_lane 1048577 at 4 lanes"),
        (dict(spp_lane=(1 << 10) + 1, lanes=4096), dict(integrator=-1, work=None), "spp_lane 1025 at 4096 lanes"),
        # 5. the integrator
        (dict(integrator=1), dict(lanes=128, flags=4, first_stream=far, work=None), "integrator 1 is out of scope"),
        (dict(integrator=3), dict(flags=1, first_stream=far), "integrator 3 is out of scope"),
        (dict(integrator=-1), dict(lanes=1), "integrator -1"),
        # 6. the flags
        (dict(flags=api.QUERY_REORDER), dict(first_stream=far, lanes=128, work=None), "PT_QUERY_REORDER"),
        (dict(flags=api.QUERY_REORDER | api.QUERY_STREAM_PAD), {}, "PT_QUERY_REORDER"),
        (dict(flags=4), dict(first_stream=far), "unknown flag bits 0x4"),
        (dict(flags=0x80000002), dict(lanes=128, work=None), "unknown flag bits 0x80000000"),
        # 7. the stream range, without PT_QUERY_STREAM_PAD
        (dict(first_stream=(1 << 31) - 4 * N + 1), {}, "pass 2^31"),
        (dict(first_stream=far), dict(lanes=128, work=None), "pass 2^31"),
        (dict(n=1 << 26, first_stream=(1 << 31) - (1 << 28) + 1), {}, "pass 2^31"),
    ]

    def args(a):
        return (a["scene"], a["n"], a["recs"], a["lanes"], a["spp_lane"], a["max_depth"], a["integrator"], a["use_mis"], a["seed"], a["first_stream"],
                a["out"])

    for change, also, msg in cases:
        for extra in ({}, also):
            a = dict(good, **extra)
            a.update(change)
            assert L.pt_query_sh(*args(a), a["flags"]) == -1, (change, extra)
            assert WALK + ": " in _err(api) and msg in _err(api), (change, extra, _err(api))
            assert L.pt_query_sh_device(*args(a), a["work"], a["flags"], None) == -1, (change, extra)
            assert WALK + ": " in _err(api) and msg in _err(api), (change, extra, _err(api))
    # 8. the device form: more than 64 lanes without a workspace; 64 lanes need none, and the next check (the device's) answers
    for lanes in (128, 4096):
        a = dict(good, lanes=lanes, work=None)
        assert L.pt_query_sh_device(*args(a), None, 0, None) == -1
        assert WALK + ": " in _err(api) and "lanes %d needs a workspace" % lanes in _err(api), _err(api)
    a = dict(good, lanes=128, work=None, flags=api.QUERY_STREAM_PAD, first_stream=far)      # with the pad flag the stream range is not checked
    assert L.pt_query_sh_device(*args(a), None, a["flags"], None) == -1 and "needs a workspace" in _err(api)
    # n == 0: 0 with a NULL scene, whatever else is passed; nothing is looked at or written
    for z in ((None, 0, None, 0, 0, 0, 7, 0, 0, 0, None), (s, 0, r, 4, 2, 8, 0, 1, 1, 0, o), (None, 0, None, 128, 0, 0, 7, 0, 0, 0, None)):
        assert L.pt_query_sh(*z, 0xff) == 0 and L.pt_query_sh_device(*z, None, 0xff, None) == 0
    assert (out == 77).all() and (work == 78).all() and not fake.any()
    sc = api.Scene.__new__(api.Scene)                          # no device scene: the checks fire before it is looked at
    sc.h = None
    with pytest.raises(api.PtError, match="pt_query_sh: null scene"):
        sc.query_sh(recs, 4, 2, 8)
    with pytest.raises(api.PtError, match="pt_query_sh: n 5 at 1073741824 lanes"):
        sc.query_sh(recs, 1 << 30, 2, 8)
    assert sc.query_sh(np.zeros((0, 8), np.float32), 4, 2, 8).shape == (0, 9, 4)


def test_sh_rays_argument_checks_in_order(api):
    """pt_query_sh_rays_device has the checks of the list that its arguments can fail, in the same order."""
    L = api.lib()
    recs, out, _, fake = _buffers()
    off = np.zeros(N * 64, np.uint32)
    r, o, s, d = recs.ctypes.data, out.ctypes.data, fake.ctypes.data, off.ctypes.data
    good = dict(scene=s, n=N, recs=r, lanes=4, seed=1, first_stream=0, off=d, rays=o, flags=0)
    far = 0xffffffff
    cases = [
        (dict(n=-1), dict(scene=None, lanes=3, flags=4, first_stream=far), "n -1 at"),
        (dict(n=(1 << 26) + 1), dict(recs=None, flags=1), "n 67108865 at 4 lanes must be 0..268435456"),
        (dict(scene=None), dict(lanes=3, flags=4, first_stream=far), "null scene"),
        (dict(recs=None), dict(lanes=0, flags=4), "null records"),
        (dict(rays=None), dict(lanes=8192, flags=1), "null output buffer"),
        (dict(lanes=0), dict(flags=4, first_stream=far), "lanes 0 must be a power of two in 1..4096"),
        (dict(lanes=6), dict(flags=1), "lanes 6 must be"),
        (dict(lanes=8192), {}, "lanes 8192 must be"),
        (dict(flags=api.QUERY_REORDER), dict(first_stream=far), "PT_QUERY_REORDER"),
        (dict(flags=8), dict(first_stream=far), "unknown flag bits 0x8"),
        (dict(first_stream=(1 << 31) - 4 * N + 1), {}, "pass 2^31"),
        (dict(first_stream=far, lanes=4096), {}, "pass 2^31"),
    ]
    for change, also, msg in cases:
        for extra in ({}, also):
            a = dict(good, **extra)
            a.update(change)
            got = L.pt_query_sh_rays_device(a["scene"], a["n"], a["recs"], a["lanes"], a["seed"], a["first_stream"], a["off"], a["rays"], a["flags"], None)
            assert got == -1, (change, extra)
            assert RAYS + ": " in _err(api) and msg in _err(api), (change, extra, _err(api))
    assert L.pt_query_sh_rays_device(None, 0, None, 0, 0, 0, None, None, 0xff, None) == 0
    assert (out == 77).all() and not fake.any()


def test_record_builders_and_the_grids_order(api):
    from cudapathtracer_amd import rays
    p = np.array([(0.5, -0.25, 1.5), (1.0, 2.0, 3.0)], np.float32)
    r = rays.sh_records(p, 7.5)
    assert r.shape == (2, 8) and r.dtype == np.float32
    assert np.array_equal(r[:, 0:3].view(np.uint32), p.view(np.uint32)) and (r[:, 3] == 7.5).all() and not r[:, 4:].view(np.uint32).any()
    assert (rays.sh_records(p)[:, 3] == np.float32(999999.0)).all()
    assert np.array_equal(rays.sh_records(p, 7.5, device="cpu").numpy().view(np.uint32), r.view(np.uint32))
    g = rays.sh_grid((0.0, 10.0, 100.0), (1.0, 12.0, 103.0), (2, 3, 4), 5.0)
    assert g.shape == (24, 8) and (g[:, 3] == 5.0).all() and not g[:, 4:].view(np.uint32).any()
    for ix in range(2):
        for iy in range(3):
            for iz in range(4):
                assert tuple(g[(iz * 3 + iy) * 2 + ix, :3]) == (float(ix), 10.0 + iy, 100.0 + iz), (ix, iy, iz)
    assert np.array_equal(g[:3, 0], np.array([0.0, 1.0, 0.0], np.float32))                       # x fastest
    one = rays.sh_grid((1.0, 2.0, 3.0), (9.0, 9.0, 9.0), (1, 1, 1))
    assert one.shape == (1, 8) and tuple(one[0, :3]) == (1.0, 2.0, 3.0)
    assert np.array_equal(rays.sh_grid((0, 0, 0), (1, 1, 1), (2, 2, 2), device="cpu").numpy(), rays.sh_grid((0, 0, 0), (1, 1, 1), (2, 2, 2)))


def _sphere_rule(nz=16, nphi=32):
    """(directions [m, 3] float64, weights [m]) of a Gauss-Legendre rule in z times a uniform rule in the azimuth: exact for the
    products of two polynomials of degree 2 and more."""
    z, wz = np.polynomial.legendre.leggauss(nz)
    phi = (np.arange(nphi) + 0.5) * (2.0 * np.pi / nphi)
    zz, pp = np.meshgrid(z, phi, indexing="ij")
    s = np.sqrt(1.0 - zz * zz)
    d = np.stack([s * np.cos(pp), s * np.sin(pp), zz], -1).reshape(-1, 3)
    w = np.repeat(wz, nphi) * (2.0 * np.pi / nphi)
    assert abs(w.sum() - 4.0 * np.pi) < 1e-12
    return d, w


def test_sh_basis_is_orthonormal_and_agrees_with_the_f32_restatement(api):
    from cudapathtracer_amd import rays
    d, w = _sphere_rule()
    y = rays.sh_basis(d)
    assert y.shape == (len(d), 9) and y.dtype == np.float64
    gram = (y * w[:, None]).T @ y
    print("max |gram - 1|", np.abs(gram - np.eye(9)).max())
    assert np.abs(gram - np.eye(9)).max() < 1e-6                  # the constants carry seven digits
    d32 = d.astype(np.float32)
    y32 = rays.sh_basis(d32)
    assert y32.dtype == np.float32 and np.abs(y32 - SR.basis(d32)).max() < 1e-6
    import torch
    assert np.allclose(rays.sh_basis(torch.from_numpy(d)).numpy(), y, rtol=0, atol=1e-15)


def test_sh_irradiance_of_a_band_limited_field(api):
    """L(d) = 1 + 0.5 d.y + 0.25 (3 d.z^2 - 1) lies in the span of the nine terms, so the convolution with the cosine lobe is exact:
    E(n) = pi + (pi / 3) n.y + (pi / 16) (3 n.z^2 - 1)."""
    from cudapathtracer_amd import rays
    d, w = _sphere_rule()
    field = 1.0 + 0.5 * d[:, 1] + 0.25 * (3.0 * d[:, 2] ** 2 - 1.0)
    coeff = (rays.sh_basis(d) * (field * w)[:, None]).sum(0)                                   # the radiance coefficients
    samples = 4096
    sums = np.zeros((2, 9, 4))
    sums[0, :, :3] = (coeff * samples / (4.0 * np.pi))[:, None]                               # what pt_query_sh would have summed
    sums[1, :, 1] = 2.0 * sums[0, :, 1]
    rng = np.random.default_rng(5)
    nrm = np.concatenate([np.eye(3), -np.eye(3), rng.standard_normal((6, 3))], 0)
    nrm /= np.linalg.norm(nrm, axis=1)[:, None]
    e = rays.sh_irradiance(sums, samples, nrm)
    want = np.pi + (np.pi / 3.0) * nrm[:, 1] + (np.pi / 16.0) * (3.0 * nrm[:, 2] ** 2 - 1.0)
    assert e.shape == (2, 12, 3)
    print("max error", np.abs(e[0] - want[:, None]).max())
    assert np.abs(e[0] - want[:, None]).max() < 1e-5
    assert np.abs(e[1, :, 1] - 2.0 * want).max() < 2e-5 and not e[1, :, 0].any() and not e[1, :, 2].any()
    import torch
    assert np.allclose(rays.sh_irradiance(torch.from_numpy(sums), samples, torch.from_numpy(nrm)).numpy(), e, rtol=0, atol=1e-12)


def test_the_map_is_onto_the_unit_sphere_and_uniform_in_z():
    """On a grid of (u1, u2) that includes 0 and values the clamp catches: |d| is within 4 ulp of 1, and d.z is 2 (1 - u1) - 1 (in
    float64, from the clamped u1) within 2 ulp; the ulp is 1's, 2^-23, d.z lying in [-1, 1]."""
    u1 = np.concatenate([np.linspace(0.0, 1.0, 257), [1e-7, 1e-3, 0.999, 1.0 - 1e-5, 1.0 - 1e-6, np.nextafter(np.float32(1.0), np.float32(0.0))]]).astype(np.float32)
    u2 = np.concatenate([np.linspace(0.0, 1.0, 64, endpoint=False), [np.nextafter(np.float32(1.0), np.float32(0.0))]]).astype(np.float32)
    a, b = (v.ravel() for v in np.meshgrid(u1, u2, indexing="ij"))
    w = SR.local_direction(a, b)
    d = SR.sphere_map(w)
    assert d.dtype == np.float32 and d.shape == (len(a), 3)
    ulp = 2.0 ** -23
    norm = np.sqrt((d.astype(np.float64) ** 2).sum(1))
    clamped = np.minimum(a, np.float32(1.0) - SR.EPS).astype(np.float64)
    z = 2.0 * (1.0 - clamped) - 1.0
    print("max | |d| - 1 | / ulp", np.abs(norm - 1.0).max() / ulp, "max |d.z - z| / ulp", np.abs(d[:, 2] - z).max() / ulp)
    assert np.abs(norm - 1.0).max() <= 4 * ulp
    assert np.abs(d[:, 2].astype(np.float64) - z).max() <= 2 * ulp
    assert d[:, 2].min() >= -1.0 and d[:, 2].max() == 1.0                                       # u1 = 0 is the pole +z; -z is left out
    assert d[:, 2].min() <= -1.0 + 4e-5
    # the azimuth is w's
    mid = (a > 0.01) & (a < 0.99)
    assert np.abs(np.arctan2(d[mid, 1], d[mid, 0]) - np.arctan2(w[mid, 1], w[mid, 0])).max() < 1e-6


def test_the_tree_on_a_hand_worked_example():
    """L = 4, values chosen so that the order of the sums shows: in f32, (2^24 + 0) + (1 + 1) is 2^24 + 2, and 2^24 when the ones
    are added to 2^24 one after the other."""
    big = np.float32(2.0 ** 24)
    a = np.zeros((1, 4, 9, 3), np.float32)
    a[0, :, 0, 0] = (big, 0.0, 1.0, 1.0)
    a[0, :, 8, 2] = (1.0, big, 1.0, 0.0)               # (1 + big) + (1 + 0) = big + 1 -> big (ties to even)
    a[0, :, 4, 1] = (0.5, 0.25, 0.125, 0.0625)
    c = SR.coeffs(a)
    assert c.shape == (1, 9, 4) and c.dtype == np.float32 and not c[..., 3].any()
    assert c[0, 0, 0] == big + np.float32(2.0) and SR.left_to_right(a)[0, 0, 0] == big
    assert c[0, 8, 2] == big and c[0, 4, 1] == np.float32(0.9375)
    assert np.count_nonzero(c) == 3
    t = SR.terms(np.array([[2.0, 0.5, 0.0, 9.0]], np.float32), np.array([[0.0, 0.0, 1.0]], np.float32))
    assert t.shape == (1, 9, 3) and t[0, 0, 0] == np.float32(2.0) * SR.C0 and t[0, 2, 1] == np.float32(0.5) * SR.C1 and not t[0, :, 2].any()
    assert t[0, 6, 0] == np.float32(2.0) * (SR.C3 * np.float32(2.0)) and not t[0, [1, 3, 4, 5, 7, 8]].any()
    two = SR.lane_sum([t, t])
    assert np.array_equal(two, (t + t).astype(np.float32))


# DESIGN.md §27's table: kernel -> (VGPRs, scratch bytes per lane, spilled VGPRs, LDS bytes per workgroup, waves per SIMD it is launched at)
TABLE = {
    "sh_naive_simple": (79, 0, 0, 47104, 3), "sh_naive_lean": (96, 0, 0, 51200, 3), "sh_naive_generic": (96, 0, 0, 51200, 3),
    "sh_mis_simple": (91, 0, 0, 47104, 3), "sh_mis_lean": (119, 0, 0, 51200, 3), "sh_mis_generic": (131, 0, 0, 51200, 3),
}


def test_each_sh_kernel_fits_the_waves_it_declares():
    """What the compile gives, pinned as tests/test_query_irradiance_api.py pins irradiance_kernel's: each of the six kernels fits
    the waves per SIMD it is launched at (3: its LDS is the class's 16 or 20 KB and 30 720 bytes of sums) in VGPRs and LDS, and needs
    no scratch there."""
    from conftest import ROOT
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import radiance_time
    import sh_time
    res, waves = sh_time.sh_kernel_resources(), sh_time.declared_waves()
    print(res, waves)
    assert set(res) == set(TABLE) == set(waves)
    rad = radiance_time.declared_waves()
    for k, (vgprs, scratch, spills, lds, w) in TABLE.items():
        r = res[k]
        assert waves[k] == w == min(rad[k.replace("sh_", "radiance_")], 3), (k, waves[k])
        assert r["vgpr_count"] == vgprs and r["private_segment_fixed_size"] == scratch and r["vgpr_spill_count"] == spills, (k, r)
        assert r["group_segment_fixed_size"] == lds == (16384 if k.endswith("simple") else 20480) + 4 * 30 * 64 * 4, (k, r)
        fit = min(512 // ((r["vgpr_count"] + 7) // 8 * 8), (160 * 1024) // r["group_segment_fixed_size"], 8)
        assert fit >= w, (k, r, fit)
