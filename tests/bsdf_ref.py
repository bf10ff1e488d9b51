"""Float64 restatement of the reference's BSDF dispatchers (reflectors.cuh:547-666), with error bounds.

Written from the reference's formulas, NOT from oracle/oracle_render.cpp: this module is the independent leg that the
oracle (tests/test_bsdf_ref_cpu.py) and the HIP probes (tests/test_bsdf_edges.py) are both held to.

    evaluate(table, material, wi, wo, eta_i)            -> f_eval + pdf_eval          (:547-584, :633-666)
    sample(table, material, wi, backface, eta_i, u)     -> sample_f_eval              (:588-629)

`wi` points INTO the surface (the dispatchers negate it, :570 / :614 ...). `u` holds the uniform draws of the case's
subsequence, in order (oracle.xorwow_uniform; the generator is pinned by tests/golden/xorwow_kat.json), so sampling is as
deterministic in float64 as it is in binary32. `dtype=np.float32` evaluates the same statements with every intermediate
rounded to binary32, operations in the written order.

Every quantity is a `V`: its value and, in float64 mode, a first-order running bound `a` of its absolute error in a binary32
evaluation, in units of 2^-24. The bound is made from the float64 values alone. For an output `x`, kappa = x.a / |x.v| is
its condition number: it is the sum, carried through the formulas, of the amplification factors of every cancelling step,
  1/denom                       D_GGX's  cos^2 (alpha^2 - 1) + 1                       (:82)
  sum|terms| / |sum|            dot(wi, h), dot(wo, h), wi + wo before normalize       (:138,:147,:157)
  1/(1 - c^2) and 1/c           the tangent in G1_GGX                                  (:95)
  1/|cosThetaT2|                the refracted z                                        (:322, :349)
and of three more that the reference's formulas have and that list leaves out:
  (t1 + t2) / |t1 - t2|         Fresnel_Conductor's Rs as it goes to 0 (eta = 1, k = 0) (:126)
  (a2plusb2 + |t0|) / |sum|     `a2plusb2 + t0` under the root of `a`: with k = 0 and eta^2 < sin^2 it is |t0| + t0 = 0, so `a`
                                is the root of a rounding error (up to 2^-12 absolute); `V.sqrt` bounds it by sqrt(a / 2^-24) (:118)
  1/(1 - |c|)                   Schlick's (1 - |cos|)^5 where R0 = 0 (index-matched leaf) (:187)
Each data-dependent decision on a computed value is recorded with its margin |x - threshold| / x.a (`Trace.decide`); a
decision on an input (wi.z <= 0, wo.z * wi.z > 0, the sign of wi.z + wo.z) is exact in binary32 and has no margin.

Tolerance of one output of one case: C * 2^-24 * x.a ( = C * 2^-24 * kappa * |x| ), C per output group below.

Quirks of the reference that are kept (each is marked `QUIRK` where it happens):
  PI = 3.141592f, EPSILON = 1e-5f as binary32 values; Fresnel_Conductor returns Rs only; G1_GGX's rational fit below a = 1.6;
  the metal sampler mirrors wo.z <= 0 upwards, the leaf sampler does not; cosine_sample_f clamps u1; the max(., EPSILON)
  floors; dielectric f_eval writes nothing and its pdf is 0; the dielectric sampler uses mat.ior and backface only, clamps
  cosThetaI to [EPSILON, 1], reflects when cosThetaT2 < 0 or F >= 0.99999 and does not normalise the refracted wo; leaf_pdf
  clamps F, leaf_sample_f does not; transmission and albedo come from the row (the probes pass uv = (0, 0); tables carry no
  textures, and a 0 x 0 texture leaves the row's albedo, oracle/README.md App. D).
"""
import os
import sys

import numpy as np

EPS24 = 2.0 ** -24


def lit(x):
    """A C `float` literal as the binary32 value it denotes."""
    return float(np.float32(x))


PI = lit(3.141592)           # QUIRK util.cuh: PI is 3.141592f, not pi
EPSILON = lit(1e-5)          # QUIRK util.cuh: EPSILON 1e-5f
U1_MAX = float(np.float32(1.0) - np.float32(EPSILON))          # `1.0f - EPSILON` (:25) is a binary32 constant expression

MAT_DIFFUSE, MAT_METAL, MAT_SMOOTHDIELECTRIC, MAT_LEAF, MAT_DELTAMIRROR = 0, 1, 2, 4, 6

# Printed by `python tests/bsdf_ref.py --measure` (section "C"): 4 x the largest |ref32 - ref64| / (2^-24 * a) of this module's
# own binary32 evaluation over every case set of tests/bsdf_cases.py. Neither the oracle nor the kernels were consulted.
C_F = 4.0
C_PDF = 4.0
C_WO = 3.3
C_WEIGHT = 4.8

BRANCH_GUARD = 64.0          # a case is left out when its smallest margin is below BRANCH_GUARD * 2^-24 (in units of x.a)
ILL_CONDITIONED = 1e-2       # f / pdf are left out when tol > ILL_CONDITIONED * |ref64|; the weight is still compared (weight_resolved)


class V:
    """value + running absolute error bound (units of 2^-24 of a binary32 evaluation); a is None in binary32 mode."""
    __slots__ = ("v", "a")

    def __init__(self, v, a=None):
        self.v, self.a = v, a

    def _c(self, o):
        if isinstance(o, V):
            return o
        return V(self.v.dtype.type(o), None if self.a is None else 0.0)

    def __add__(self, o):
        o = self._c(o); v = self.v + o.v
        return V(v, None if self.a is None else self.a + o.a + np.abs(v))

    def __sub__(self, o):
        o = self._c(o); v = self.v - o.v
        return V(v, None if self.a is None else self.a + o.a + np.abs(v))

    def __mul__(self, o):
        o = self._c(o); v = self.v * o.v
        return V(v, None if self.a is None else np.abs(self.v) * o.a + np.abs(o.v) * self.a + np.abs(v))

    def __truediv__(self, o):
        o = self._c(o); v = self.v / o.v
        return V(v, None if self.a is None else (self.a + np.abs(v) * o.a) / np.abs(o.v) + np.abs(v))

    def __radd__(self, o): return self._c(o) + self
    def __rsub__(self, o): return self._c(o) - self
    def __rmul__(self, o): return self._c(o) * self
    def __rtruediv__(self, o): return self._c(o) / self
    def __neg__(self): return V(-self.v, self.a)
    def abs(self): return V(np.abs(self.v), self.a)

    def sqrt(self):
        v = np.sqrt(self.v)
        if self.a is None:
            return V(v)
        # |sqrt(x + d) - sqrt(x)| <= min(d / (2 sqrt x), sqrt d): the second arm is what is left when x cancels to 0
        return V(v, np.fmin(self.a / (2.0 * v), np.sqrt(self.a / EPS24)) + v)

    def rsqrt(self):
        v = self.v.dtype.type(1.0) / np.sqrt(self.v)
        return V(v, None if self.a is None else self.a * np.abs(v) / (2.0 * np.abs(self.v)) + np.abs(v))

    def pow5(self):          # powf(x, 5.0f)
        v = (self.v.astype(np.float64) ** 5).astype(self.v.dtype)
        return V(v, None if self.a is None else 5.0 * self.v ** 4 * self.a + np.abs(v))

    def sin(self):
        v = np.sin(self.v)
        return V(v, None if self.a is None else np.abs(np.cos(self.v)) * self.a + np.abs(v))

    def cos(self):
        v = np.cos(self.v)
        return V(v, None if self.a is None else np.abs(np.sin(self.v)) * self.a + np.abs(v))

    def fmax(self, c):       # fmaxf(x, c) with a constant: a NaN x gives c
        c = self.v.dtype.type(c); v = np.fmax(self.v, c)
        return V(v, None if self.a is None else np.where(self.v > c, self.a, 0.0))

    def fmin(self, c):
        c = self.v.dtype.type(c); v = np.fmin(self.v, c)
        return V(v, None if self.a is None else np.where(self.v < c, self.a, 0.0))


def where(c, x, y):
    return V(np.where(c, x.v, y.v), None if x.a is None else np.where(c, x.a, y.a))


def vec(dt, arr):
    """exact inputs: n x 3 binary32 -> three V"""
    a = np.asarray(arr, np.float32).astype(dt)
    return [V(np.ascontiguousarray(a[:, i]), None if dt == np.float32 else np.zeros(len(a))) for i in range(3)]


def scal(dt, arr):
    a = np.asarray(arr, np.float32).astype(dt)
    return V(a, None if dt == np.float32 else np.zeros(a.shape))


def dot(a, b):               # util.cuh:116-118, left to right
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def normalize(v):            # util.cuh:128-131: v * rsqrtf(dot(v, v)); normalize(0) is NaN
    inv = dot(v, v).rsqrt()
    return [v[0] * inv, v[1] * inv, v[2] * inv]


class Trace:
    """Collects the margin of every data-dependent decision that a case really reaches."""

    def __init__(self, n, track):
        self.track = track
        self.margin = np.full(n, np.inf)
        self.which = np.full(n, -1)
        self.names = []
        self.soft = {}

    def margin_of(self, x, thr):
        with np.errstate(all="ignore"):
            m = np.abs(x.v - thr) / x.a
        # an input compared with a constant (a = 0) and an infinite / NaN operand are decided alike in both precisions
        m = np.where(np.isfinite(x.v) & (x.a > 0), m, np.inf)
        return np.where(np.isnan(m), 0.0, m)

    def note(self, name, m, reached):
        """a continuous switch: its margin is reported (`soft`), the case stays in"""
        self.soft[name] = np.where(reached, m, np.inf)

    def decide(self, name, x, thr, taken, reached):
        """`taken` = the decision as made from x.v; x is compared with thr where `reached`."""
        if not self.track:
            return taken
        m = np.where(reached, self.margin_of(x, thr), np.inf)
        if name not in self.names:
            self.names.append(name)
        low = m < self.margin
        self.margin = np.where(low, m, self.margin)
        self.which = np.where(low, self.names.index(name), self.which)
        return taken


def read_table(materials):
    """176-byte Material rows (objects.cuh:605-638) -> the fields the BSDFs read."""
    m = np.ascontiguousarray(materials).view(np.uint8).reshape(-1, 176)
    f = m.view(np.float32)
    return dict(type=m.view(np.int32)[:, 8].copy(), albedo=f[:, 12:15].copy(), roughness=f[:, 16].copy(), eta=f[:, 20:23].copy(),
                k=f[:, 24:27].copy(), ior=f[:, 28].copy(), transmission=f[:, 31].copy())


# ---- the arms --------------------------------------------------------------------------------------------------------

def cosine_f(albedo):        # :10-13
    return [c / PI for c in albedo]


def cosine_pdf(z):           # :15-18  QUIRK max(z, EPSILON)
    return z.fmax(EPSILON) / PI


def cosine_sample(u1, u2):   # :21-39
    u1 = u1.fmin(U1_MAX)                                        # QUIRK u1 clamp
    r = u1.sqrt()
    phi = (2.0 * PI) * u2
    return [r * phi.cos(), r * phi.sin(), (1.0 - u1).sqrt()]


def D_GGX(hz, alpha):        # :78-84
    alpha2 = alpha * alpha
    denom = hz * hz * (alpha2 - 1.0) + 1.0
    return alpha2 / (PI * denom * denom)


def G1_GGX(c, alpha, tr, reached, name):    # :92-101  QUIRK the rational fit below a = 1.6, 1 above
    tan = (1.0 - c * c).sqrt() / c
    at = alpha * tan
    a = 1.0 / at
    small = a.v < a.v.dtype.type(lit(1.6))
    fit = (lit(3.535) * a + lit(2.181) * a * a) / (1.0 + lit(2.276) * a + lit(2.577) * a * a)
    g = where(small, fit, a._c(1.0))
    if g.a is not None:
        # The fit meets 1 at a = 1.6 (fit(1.6) = 1.00006), so this switch is continuous: a binary32 run that takes the other arm
        # is off by no more than |fit(a) - 1| + fit's own bound. That is added where the margin is short; nothing is left out.
        # a < 1.6 is alpha tan > 1/1.6 up to the quotient's rounding: where tan itself cancels to nothing (near the normal)
        # `a` has no relative accuracy left, yet alpha tan is nowhere near 0.625 and the arm is certain
        m = np.fmax(tr.margin_of(a, lit(1.6)), tr.margin_of(V(at.v, at.a + np.abs(at.v)), 1.0 / lit(1.6)))
        tr.note(name, m, reached)
        g = V(g.v, np.where(m < BRANCH_GUARD * EPS24, g.a + fit.a + np.abs(fit.v - 1.0) / EPS24, g.a))
    return g


def fresnel_conductor(c, eta, k):           # :108-127  QUIRK returns Rs only (Rp is computed and dropped)
    c2 = c * c
    s2 = 1.0 - c2
    out = []
    for e, kk in zip(eta, k):
        eta2 = e * e
        k2 = kk * kk
        t0 = eta2 - k2 - s2
        a2plusb2 = (t0 * t0 + 4.0 * eta2 * k2).sqrt()
        t1 = a2plusb2 + c2
        a = (0.5 * (a2plusb2 + t0)).sqrt()
        t2 = 2.0 * c * a
        out.append((t1 - t2) / (t1 + t2))
    return out


def schlick(c, etaI, etaT):  # :183-188
    R0 = (etaI - etaT) / (etaI + etaT)
    R0 = R0 * R0
    return R0 + (1.0 - R0) * (1.0 - c.abs()).pow5()


def half_vector(wi, wo):
    return normalize([wi[0] + wo[0], wi[1] + wo[1], wi[2] + wo[2]])


def microfacet_metal(eta, k, rough, wi, wo, tr, reached):
    """microfacet_metal_f (:129-150), microfacet_pdf (:152-158) and the weight f |wo.z| / pdf with D cancelled."""
    zero = wi[2]._c(0.0)
    dead = (wi[2].v <= 0) | (wo[2].v <= 0)                      # :131; wo.z of a SAMPLED wo is decided in sample()
    h = half_vector(wi, wo)
    hz_pdf = h[2]
    flip = h[2].v <= 0                                          # :140 — the sign of wi.z + wo.z, exact in binary32
    hf = [where(flip, -x, x) for x in h]
    alpha = rough * rough
    D = D_GGX(hf[2], alpha)
    live = reached & ~dead
    G = G1_GGX(wi[2], alpha, tr, live, "a(wi) - 1.6") * G1_GGX(wo[2], alpha, tr, live, "a(wo) - 1.6")
    Fr = fresnel_conductor(dot(wi, hf), eta, k)
    den = (4.0 * wi[2] * wo[2]).fmax(EPSILON)                   # QUIRK floor
    f = [where(dead, zero, (D * G * F) / den) for F in Fr]
    pdf = (D_GGX(hz_pdf, rough * rough) * hz_pdf) / (4.0 * dot(wo, h))
    # f |wo.z| / pdf = G F |wo.z| 4 dot(wo, h) / (den h.z): D is the same expression of h.z^2 in both and cancels
    w = [where(dead, zero / pdf, (G * F) / den * wo[2].abs() * (4.0 * dot(wo, h)) / hz_pdf) for F in Fr]
    return f, pdf, w, hz_pdf / (4.0 * dot(wo, h))


def leaf(albedo, ior, currIOR, rough, trans, wi, wo, tr, reached):
    """leaf_f (:420-461) and leaf_pdf (:463-506)."""
    refl = (wo[2].v * wi[2].v) > 0                              # :422 — a product's sign is exact in binary32
    F = schlick(wi[2], currIOR, ior)                            # :427
    h = half_vector(wi, wo)
    mF = schlick(dot(wi, h), currIOR, ior)                      # :432, before the flip
    hf = [where(h[2].v <= 0, -x, x) for x in h]                 # :436
    alpha = rough * rough
    D = D_GGX(hf[2], alpha)
    live = reached & refl
    G = G1_GGX(wi[2], alpha, tr, live, "a(wi) - 1.6") * G1_GGX(wo[2], alpha, tr, live, "a(wo) - 1.6")
    cut = D * G * mF / (4.0 * wi[2] * wo[2]).fmax(EPSILON)
    dif = cosine_f(albedo)
    f_r = [(1.0 - mF) * (1.0 - trans) * d + cut for d in dif]   # :454
    f_t = [d * (trans * (1.0 - F)) for d in dif]                # :458-459
    f = [where(refl, a, b) for a, b in zip(f_r, f_t)]
    Fp = schlick(wi[2].abs(), currIOR, ior)                     # :470
    cap = 1.0 - lit(0.1) * rough
    Fp = where(Fp.v < cap.v, Fp, cap)                           # :472  QUIRK leaf_pdf clamps F, leaf_sample_f does not
    hp = [where(h[2].v < 0, -x, x) for x in h]                  # :481 (`<`, not `<=`)
    pdf_c = (D_GGX(hp[2], alpha) * hp[2]) / (4.0 * dot(wo, hp))
    pdf_r = (Fp * pdf_c) + (((1.0 - Fp) * (1.0 - trans)) * cosine_pdf(wo[2]))
    pdf_t = cosine_pdf(-wo[2]) * ((1.0 - Fp) * trans)
    return f, where(refl, pdf_r, pdf_t)


def _rows(dt, T, material):
    g = lambda k: T[k][material]
    return (g("type"), vec(dt, g("albedo")), scal(dt, g("roughness")), vec(dt, g("eta")), vec(dt, g("k")), scal(dt, g("ior")),
            scal(dt, g("transmission")))


def _pick(types, arms, like):
    out = V(np.zeros_like(like.v), None if like.a is None else np.zeros(like.v.shape))
    for t, x in arms.items():
        out = where(types == t, x, out)
    return out


def _eval(dt, T, material, wi_in, wo, eta_i, tr, reached=None):
    """f_eval (:547-584) and pdf_eval (:633-666) on V inputs; wi_in points into the surface."""
    ty, albedo, rough, eta, k, ior, trans = _rows(dt, T, material)
    n = len(ty)
    reached = np.ones(n, bool) if reached is None else reached
    wi = [-c for c in wi_in]
    etaI = scal(dt, np.full(n, eta_i, np.float32))
    one = V(np.ones(n, dt), None if dt == np.float32 else np.zeros(n))
    with np.errstate(all="ignore"):
        mf, mpdf, mw, mq = microfacet_metal(eta, k, rough, wi, wo, tr, reached & (ty == MAT_METAL))
        lf, lpdf = leaf(albedo, ior, etaI, rough, trans, wi, wo, tr, reached & (ty == MAT_LEAF))
        df = cosine_f(albedo)                                   # :566
        dpdf = cosine_pdf(wo[2])
        mirror = one / wo[2].fmax(EPSILON)                      # :59-63
        f = [_pick(ty, {MAT_DIFFUSE: df[i], MAT_METAL: mf[i], MAT_LEAF: lf[i], MAT_DELTAMIRROR: mirror}, one) for i in range(3)]
        # QUIRK :572-575 / :654-657 the dielectric arm of f_eval writes nothing (the probe's f starts at 0) and its pdf is 0
        pdf = _pick(ty, {MAT_DIFFUSE: dpdf, MAT_METAL: mpdf, MAT_LEAF: lpdf, MAT_DELTAMIRROR: one}, one)
        az = wo[2].abs()
        w = [where(ty == MAT_METAL, mw[i], f[i] * az / pdf) for i in range(3)]
    # what the weight divides by: the pdf, for a metal its D-free factor. Where binary32 cannot tell it from 0 the quotient
    # f |wo.z| / pdf is 0/0 or x/0 there and carries no information (`weight_resolved`)
    return f, pdf, w, where(ty == MAT_METAL, mq, pdf)


def _pack(dt, tr, **groups):
    out = {}
    for name, vs in groups.items():
        vs = vs if isinstance(vs, list) else [vs]
        out[name] = np.stack([x.v for x in vs], 1)
        if dt == np.float64:
            with np.errstate(all="ignore"):
                out[name + "_a"] = np.stack([np.broadcast_to(x.a, x.v.shape) for x in vs], 1)
    if dt == np.float64:
        out["margin"], out["margin_which"], out["margin_names"], out["soft_margins"] = tr.margin, tr.which, list(tr.names), dict(tr.soft)
    return out


def evaluate(table, material, wi, wo, eta_i, dtype=np.float64):
    """-> dict: f [n,3], pdf [n,1], weight [n,3] (+ `<name>_a` error bounds, margin, in float64 mode)."""
    T = read_table(table); material = np.asarray(material)
    tr = Trace(len(material), dtype == np.float64)
    f, pdf, w, q = _eval(dtype, T, material, vec(dtype, wi), vec(dtype, wo), eta_i, tr)
    return _pack(dtype, tr, f=f, pdf=pdf, weight=w, wq=q)


def sample(table, material, wi, backface, eta_i, u, dtype=np.float64):
    """sample_f_eval (:588-629). u: [n, 4] uniform draws of each case's stream.
    -> dict: wo [n,3], f [n,3], pdf [n,1], weight [n,3], draws [n] (+ bounds and margin in float64 mode)."""
    dt = dtype
    T = read_table(table); material = np.asarray(material); backface = np.asarray(backface).astype(bool)
    n = len(material)
    tr = Trace(n, dt == np.float64)
    ty, albedo, rough, eta, k, ior, trans = _rows(dt, T, material)
    wi_in = vec(dt, wi)
    wi_l = [-c for c in wi_in]
    U = [scal(dt, np.asarray(u, np.float32)[:, i]) for i in range(4)]
    etaI = scal(dt, np.full(n, eta_i, np.float32))
    one = V(np.ones(n, dt), None if dt == np.float32 else np.zeros(n)); zero = V(np.zeros(n, dt), None if dt == np.float32 else np.zeros(n))
    is_m, is_l, is_d = ty == MAT_METAL, ty == MAT_LEAF, ty == MAT_SMOOTHDIELECTRIC

    def ggx_h(u1, u2):       # :163-173 / :514-524
        alpha = rough * rough
        phi = (2.0 * PI) * u2
        ct = ((1.0 - u1) / (1.0 + (alpha * alpha - 1.0) * u1)).sqrt()
        st = (1.0 - ct * ct).fmax(0.0).sqrt()
        return [st * phi.cos(), st * phi.sin(), ct]

    def reflect(h):          # :175 / :526  wo = 2 dot(wi, h) h - wi
        d = 2.0 * dot(wi_l, h)
        return [d * h[0] - wi_l[0], d * h[1] - wi_l[1], d * h[2] - wi_l[2]]

    with np.errstate(all="ignore"):
        # diffuse (:610)
        wo_d = cosine_sample(U[0], U[1])
        # metal (:160-180)  QUIRK wo.z <= 0 is mirrored upwards
        wo_m = reflect(ggx_h(U[0], U[1]))
        # wo.z -> |wo.z| is continuous: a flip decided otherwise in binary32 moves nothing by more than wo.z's own bound
        flip = wo_m[2].v <= 0
        if tr.track:
            tr.note("metal wo.z flip", tr.margin_of(wo_m[2], 0.0), is_m)
        wo_m[2] = where(flip, -wo_m[2], wo_m[2])
        # mirror (:70-76)
        wo_s = [-wi_l[0], -wi_l[1], wi_l[2]]
        # leaf (:508-543)  QUIRK unclamped F here; wo is not mirrored
        Fl = schlick(wi_l[2], etaI, ior)
        spec = tr.decide("leaf u - F", Fl, U[0].v, U[0].v < Fl.v, is_l)
        thru = tr.decide("leaf u - transmission", trans, U[1].v, U[1].v < trans.v, is_l & ~spec)     # an input against an input: exact
        wo_ls = reflect(ggx_h(U[1], U[2]))
        wo_lc = cosine_sample(U[2], U[3])
        wo_lt = [wo_lc[0], wo_lc[1], -wo_lc[2]]
        wo_l = [where(spec, a, where(thru, b, c)) for a, b, c in zip(wo_ls, wo_lt, wo_lc)]
        # where f / pdf of a sampled leaf direction switch arms: the sign of wo.z (wi.z is an input)
        tr.decide("leaf wo.z sign", wo_l[2], 0.0, wo_l[2].v > 0, is_l)
        # dielectric (:304-369)  QUIRK mat.ior and backface only; cosThetaI clamped to [EPSILON, 1]
        eI = where(backface, ior, one); eT = where(backface, one, ior)
        ci = wi_l[2].fmax(EPSILON).fmin(1.0)
        e = eI / eT
        ct2 = 1.0 - e * e * (1.0 - ci * ci)
        Fd = schlick(ci, eI, eT)
        tir = tr.decide("cosThetaT2", ct2, 0.0, ct2.v < 0, is_d)
        full = tr.decide("F - 0.99999", Fd, lit(0.99999), Fd.v >= dt(lit(0.99999)), is_d & ~tir)     # QUIRK :328
        all_r = tir | full
        drefl = tr.decide("dielectric u - F", Fd, U[0].v, U[0].v < Fd.v, is_d & ~all_r)
        wo_r = [-wi_l[0], -wi_l[1], wi_l[2]]
        wo_t = [-e * wi_l[0], -e * wi_l[1], -(ct2.sqrt())]      # QUIRK not normalised (:346-350)
        rden = wo_r[2].fmax(EPSILON)
        f_all, f_refl = one / rden, Fd / rden
        f_tr = ((1.0 - Fd) / wo_t[2].abs().fmax(EPSILON)) * (e * e)      # :355-356, :366 (TRANSPORTMODE_RADIANCE)
        wo_di = [where(all_r | drefl, a, b) for a, b in zip(wo_r, wo_t)]
        f_di = where(all_r, f_all, where(drefl, f_refl, f_tr))
        pdf_di = where(all_r, one, where(drefl, Fd, 1.0 - Fd))

        wo = [_pick(ty, {MAT_DIFFUSE: wo_d[i], MAT_METAL: wo_m[i], MAT_SMOOTHDIELECTRIC: wo_di[i], MAT_LEAF: wo_l[i],
                         MAT_DELTAMIRROR: wo_s[i]}, one) for i in range(3)]
        # diffuse, metal and leaf evaluate f and pdf at the sampled wo (:37-38, :178-179, :541-542); diffuse uses the albedo
        # sampled at uv (:610) where f_eval uses the row's (:566) — the same without textures
        f, pdf, w, q = _eval(dt, T, material, wi_in, wo, eta_i, tr, reached=~is_d & (ty != MAT_DELTAMIRROR))
        mirror_f = one / wo_s[2].fmax(EPSILON)
        f = [where(is_d, f_di, where(ty == MAT_DELTAMIRROR, mirror_f, f[i])) for i in range(3)]
        pdf = where(is_d, pdf_di, pdf)
        q = where(is_d, pdf_di, q)
        az = wo[2].abs()
        w = [where(is_d | (ty == MAT_DELTAMIRROR), f[i] * az / pdf, w[i]) for i in range(3)]
    draws = np.select([ty == MAT_DIFFUSE, is_m, is_d, is_l], [2, 2, np.where(all_r, 0, 1), np.where(spec, 3, 4)], 0)
    out = _pack(dt, tr, wo=wo, f=f, pdf=pdf, weight=w, wq=q)
    out["draws"] = draws
    return out


# ---- comparison under the issue's sections 3 and 4 -----------------------------------------------------------------------

GROUPS = (("f", "C_F"), ("pdf", "C_PDF"), ("wo", "C_WO"), ("weight", "C_WEIGHT"))


def constants():
    return dict(f=C_F, pdf=C_PDF, wo=C_WO, weight=C_WEIGHT)


def branch_excluded(ref):
    return ref["margin"] < BRANCH_GUARD * EPS24


def ill_conditioned(ref, group, C):
    """[n, k] bool: tol > 1e-2 |ref64| (finite outputs only; applies to f and pdf)."""
    with np.errstate(all="ignore"):
        return np.isfinite(ref[group]) & (C * EPS24 * ref[group + "_a"] > ILL_CONDITIONED * np.abs(ref[group]))


def weight_resolved(ref):
    """[n, 1] bool: the divisor of the weight is away from 0 by more than twice its own tolerance."""
    with np.errstate(all="ignore"):
        return np.isfinite(ref["wq"]) & (2.0 * C_PDF * EPS24 * ref["wq_a"] < np.abs(ref["wq"]))


def ratio(ref, got, group):
    """|got - ref64| / (2^-24 * a) where ref64 is finite; NaN elsewhere."""
    with np.errstate(all="ignore"):
        r = np.abs(got[group].astype(np.float64) - ref[group]) / (EPS24 * ref[group + "_a"])
        r = np.where((got[group].astype(np.float64) == ref[group]), 0.0, r)
    return np.where(np.isfinite(ref[group]) & np.isfinite(ref[group + "_a"]), r, np.nan)


def derive_weight(out):
    """f |wo.z| / pdf in binary32 from a probe's (or the binary32 restatement's) own outputs."""
    with np.errstate(all="ignore"):
        wz = out["wo"][:, 2:3] if "wo" in out else out["wo_in"][:, 2:3]
        return (out["f"].astype(np.float32) * np.abs(wz.astype(np.float32)) / out["pdf"].astype(np.float32)).astype(np.float32)


def check(ref, got, exact=None, what="", ref32=None, cls=None):
    """Hold `got` (dict of binary32 outputs: f, pdf, [wo, draws,] weight is derived) to the float64 `ref`.

    exact: bool [n], the cases of the exact-edge set. None of them is left out by any rule: each output is compared under its
    own tolerance, however large. Where float64 or the restatement's own binary32 run (`ref32`, needed with `exact`) is not
    finite there - normalize() of an exact zero vector, x/0, 0/0 - the two precisions legitimately part and the output is
    asserted by the class the binary32 restatement defines: a NaN for a NaN (any payload or sign), an infinity by its sign.
    cls: int [n] class of each case, for the shares per class.
    Returns a dict: branch, ill, unresolved (shares of the set as before: cases left out by the branch rule, f / pdf outputs
    left out as ill-conditioned, weights not compared among the cases with a pdf); by_class {class: (branch, ill)};
    exact_by_class (number of exact outputs asserted by class) and exact_unbounded (exact outputs whose bound is not finite,
    so that nothing but finiteness is asserted of them)."""
    n = len(ref["margin"])
    ex = np.zeros(n, bool) if exact is None else np.asarray(exact, bool)
    assert ref32 is not None or not ex.any()
    skip = branch_excluded(ref) & ~ex
    got = dict(got)
    got["weight"] = derive_weight(got)
    if ref32 is not None:
        ref32 = dict(ref32)
        ref32["wo_in"] = got.get("wo_in")
        ref32["weight"] = derive_weight(ref32)
    ill_case = np.zeros(n, bool)
    ill_n = ill_tot = by_class_n = unbounded = 0
    for group, cname in GROUPS:
        if group not in got or group not in ref:
            continue
        C = constants()[group]
        r, g = ref[group], got[group].astype(np.float64)
        E = ex[:, None] & np.ones_like(r, bool)
        use = ~skip[:, None] & np.ones_like(r, bool)
        if group == "weight":
            use = use & (weight_resolved(ref) | E)
        # the exact set where the precisions part: the class of the binary32 restatement
        if ex.any():
            r32 = ref32[group].astype(np.float64)
            deg = E & (~np.isfinite(r) | ~np.isfinite(r32))
            same = (np.isnan(r32) & np.isnan(g)) | (np.isinf(r32) & (g == r32)) | (np.isfinite(r32) & np.isfinite(g))
            assert np.all(same[deg]), "%s %s: %d exact-edge outputs are not of the class the restatement defines, first case %d: got %r, binary32 %r, float64 %r" \
                % (what, group, (deg & ~same).sum(), np.argwhere(deg & ~same)[0][0], g[deg & ~same][0], r32[deg & ~same][0], r[deg & ~same][0])
            by_class_n += int(deg.sum())
            use = use & ~deg
            unbounded += int((use & E & np.isfinite(r) & ~np.isfinite(ref[group + "_a"])).sum())
        # non-finite float64 elsewhere: the class is asserted (NaN: any payload or sign; inf: exact)
        nanm = use & np.isnan(r)
        assert np.all(np.isnan(g[nanm])), "%s %s: %d NaN of the restatement are not NaN" % (what, group, (~np.isnan(g[nanm])).sum())
        infm = use & np.isinf(r)
        assert np.array_equal(g[infm], r[infm]), "%s %s: infinities differ" % (what, group)
        lim = use & np.isfinite(r)
        if group in ("f", "pdf"):
            ill = ill_conditioned(ref, group, C) & ~E
            ill_n += int((ill & lim).sum()); ill_tot += int((lim & ~E).sum())
            ill_case |= (ill & lim).any(1)
            lim = lim & ~ill
        with np.errstate(all="ignore"):
            err = np.abs(g - r)
            tol = np.where(np.isfinite(ref[group + "_a"]), C * EPS24 * ref[group + "_a"], np.inf)
        bad = lim & ~(err <= tol)
        if bad.any():
            i, j = np.argwhere(bad)[np.argmax((err / tol)[bad])]
            raise AssertionError("%s %s: %d of %d outputs off the float64 restatement; worst case %d[%d]: got %r ref %r tol %.3g (%.1f x)"
                                 % (what, group, bad.sum(), lim.sum(), i, j, g[i, j], r[i, j], tol[i, j], err[i, j] / tol[i, j]))
        zero = lim & (r == 0) & (ref[group + "_a"] == 0)
        assert np.all(g[zero] == 0), "%s %s: exact zeros differ" % (what, group)
    if "draws" in got and "draws" in ref:
        d = np.asarray(got["draws"]).astype(np.int64)
        assert np.array_equal(d[~skip], ref["draws"][~skip]), "%s: draw counts differ in %d cases" % (what, (d[~skip] != ref["draws"][~skip]).sum())
    has_pdf = np.isfinite(ref["pdf"][:, 0]) & (ref["pdf"][:, 0] != 0) & ~skip & ~ex
    unres = ~weight_resolved(ref)[:, 0] & has_pdf
    by_class = {}
    if cls is not None:
        for c in np.unique(cls[~ex]):
            m = (cls == c)
            by_class[int(c)] = (float(skip[m].mean()), float(ill_case[m & ~skip].mean()) if (m & ~skip).any() else 0.0,
                                float(unres[m].sum() / max(has_pdf[m].sum(), 1)))
    return dict(branch=float(skip.mean()), ill=(ill_n / ill_tot if ill_tot else 0.0), unresolved=float(unres.sum() / max(has_pdf.sum(), 1)),
                by_class=by_class, exact_by_class=by_class_n, exact_unbounded=unbounded)


def measure(O):
    """-> ({group: 4 x largest ratio, one decimal}, rows of (set, probe, n, branch share, ill share, per-class text))."""
    import bsdf_cases as BC
    worst = {g: 0.0 for g, _ in GROUPS}
    rows = []
    for cs in BC.all_sets(O):
        for kind in ("eval", "sample"):
            r64, r32 = BC.restate(cs, kind, np.float64), dict(BC.restate(cs, kind, np.float32))
            r32["wo_in"] = cs.wo
            r32["weight"] = derive_weight(r32)      # the weight as a probe's outputs give it, not the D-free form
            skip = branch_excluded(r64) & ~cs.exact
            ill_any = np.zeros(cs.n, bool)
            ill_n = ill_tot = 0
            for g, _ in GROUPS:
                if g not in r64:
                    continue
                q = ratio(r64, r32, g)
                q = np.where(skip[:, None] | ((~weight_resolved(r64) & ~cs.exact[:, None]) if g == "weight" else False), np.nan, q)
                if g in ("f", "pdf"):
                    ill = ill_conditioned(r64, g, constants()[g]) & ~cs.exact[:, None]
                    fin = np.isfinite(r64[g]) & ~skip[:, None]
                    ill_n += int((ill & fin).sum()); ill_tot += int(fin.sum())
                    ill_any |= (ill & fin).any(1)
                    q = np.where(ill, np.nan, q)
                if np.isfinite(q).any():
                    worst[g] = max(worst[g], float(np.nanmax(q)))
            per_class = ["%s %.1f/%.1f" % (c, 100 * skip[cs.cls == i].mean(), 100 * ill_any[cs.cls == i].mean()) for i, c in enumerate(BC.CLASSES)]
            rows.append((cs.name, kind, cs.n, float(skip.mean()), ill_n / max(ill_tot, 1), per_class))
    return {g: round(4 * worst[g], 1) for g in worst}, rows


def _measure():
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, here); sys.path.insert(0, os.path.dirname(here))
    from oracle import oracle_py as O
    O.build()
    C, rows = measure(O)
    print("## C (4 x the largest binary32-vs-float64 ratio of the restatement itself)")
    for g, cname in GROUPS:
        print("%s = %.1f    (the module has %.1f)" % (cname, C[g], constants()[g]))
    print("## share left out per set: branch rule (cap 2 %), ill-conditioned f / pdf outputs (cap 10 %); per class in % (branch/ill cases)")
    for name, kind, n, a, b, pc in rows:
        print("%-24s %-6s n=%5d  branch %.4f  ill %.4f   %s" % (name, kind, n, a, b, "  ".join(pc)))


if __name__ == "__main__":
    if "--measure" in sys.argv:
        _measure()
    else:
        print(__doc__)
