"""Host-side exact reference of the RBM family that works from the packed bits (pynqs_rbm_forward, pynqs_rbm_children_prepare +
pynqs_rbm_forward_children, pynqs_rbm_grad; include/pynqs_amd.h), an extension of mcmc_replay.Rbm from ln|psi| to the complete ln psi,
its condition number, the gradient estimator and the a-priori rounding bounds the GPU tests assert.  Everything here is computed from
the float64 parameters and the +-1 rows alone, in numpy longdouble (64-bit mantissa) with forms that neither overflow nor cancel, and
in mpmath at MP_DPS digits for spot checks; nothing depends on a kernel's output.

ln psi.   theta_h = b_h + sum_o W_ho x_o = a + i b,  s = sign(a),  e = exp(-2 |a|):
    2cosh(theta) = exp(s theta) (1 + e exp(-2 i s b)),    |1 + e exp(-2 i s b)|^2 = (1 - e)^2 + 4 e cos^2 b   (all terms >= 0),
    Re ln 2cosh  = |a| + ln((1 - e)^2 + 4 e cos^2 b) / 2    (real parameters: |a| + log1p(e)),
    Im ln 2cosh  = s b + atan2(-2 s e sin b cos b, (1 - e) + 2 e cos^2 b),
    tanh(theta)  = (s (1 - e^2) + 2 i e sin 2b) / ((1 - e)^2 + 4 e cos^2 b).
"real": psi = exp(a.x + sum_h ln 2cosh);  "tanh": tanh(a.x) exp(sum_h ln 2cosh);  "pRBM": exp(i (a.x + sum_h ln 2cosh));  "complex":
exp(a.x + sum_h ln 2cosh) with complex parameters.

Condition number and the amplitude bound.  With S_h = |b_h| + sum_o |W_ho| (moduli),
    cond(x) = 1 + sum_h |tanh theta_h| S_h + sum_o |a_o|,         |psi / psi_exact - 1| <= u (sorb + H + 16) cond(x),   u = 2^-53.
theta_h is a chain of sorb fused multiply-adds on terms of modulus <= S_h: its error is at most (sorb + 1) u S_h.  d ln 2cosh / d theta
= tanh theta turns that into (sorb + 1) u |tanh theta_h| S_h per unit; the sum over the units gives the middle term.  a.x carries
(sorb + 1) u sum_o |a_o|.  The H additions of the exponent (or the H multiplications of the bounded factors with their
renormalisations), the exponential, the sine / cosine of the phase and the final products each add a few u RELATIVE TO ln psi itself,
which is <= cond(x) because |ln 2cosh theta| <= |tanh theta| |theta| + ln 2 <= |tanh theta_h| S_h + 1: hence H + 16 more units of
u cond(x).  The children route forms the same theta-dependent quantities from exp(-2 theta) of the parent times four table entries
exp(-+4 W_ho): six roundings per unit on top of the parent's theta, covered by the same sorb + 1 per unit.
"tanh" multiplies by tanh(a.x), which crosses zero, so a bound relative to psi alone would be wrong next to the crossing: the error
of a.x, at most (sorb + 1) u sum_o |a_o|, goes through d tanh = sech^2 and is ABSOLUTE in units of prod = prod_h 2cosh, and tanh's own
rounding adds u |prod|.  Hence |psi - psi_exact| <= u (sorb + H + 16) cond(x) |psi_exact| + u ((sorb + 1) sum_o |a_o| sech^2(a.x) + 1) |prod|.
"pRBM": the bound is on the phase (and on | |psi| - 1 |), absolute.

Gradient (include/pynqs_amd.h, pynqs_rbm_grad): f_n = p_n (E_n - <E> c_n), O = (x_o, tanh theta_h, tanh theta_h x_o),
G_k = sum_n conj(f_n) O_k(x_n); the gradient is 2 Re G (real parameters) or (2 Re G, -2 Im G).  Per output k
    |G_k - G_exact_k| <= u [ 4 sum_n a_n |O_nk| + sum_n |f_n| ((40 + n / 128) max(1, |tanh theta_nh|) + (sorb + 2) S_h |sech^2 theta_nh|) ],
    a_n = p_n (|E_n| + |<E>| |c_n|);  visible-bias outputs: u [ 4 sum_n a_n + (40 + n / 128) sum_n |f_n| ].
First term: the roundings of f_n = p_n (E_n - <E> c_n) (a product, a difference of numbers near -100 Ha, a product) act on a_n, not on
|f_n|.  Second: the additions (32 walkers of a workgroup in turn, then n / 32 partial sums in four slices: 36 + n / 128 of them) and
tanh formed as (1 - e) / (1 + e), whose error is a few u absolute -- hence max(1, .), a bound relative to tanh would be wrong for
theta ~ 1e-8.  Third: the error of theta, (sorb + 1) u S_h, through d tanh / d theta = sech^2.
Loss = 2 Re sum_n conj(ln psi_n) f_n with Im ln psi on the principal branch: the same with |ln psi_n| in place of |O_nk|, plus the
amplitude bound u (sorb + H + 16) cond(x_n) |f_n| per walker, all times the loss' factor 2."""
from __future__ import annotations

from dataclasses import dataclass

import mpmath
import numpy as np

from mcmc_replay import MP_DPS, MP_WORK, Rbm, pm1  # noqa: F401  (pm1, MP_WORK: for the tests that import this module)

LD, CLD = np.longdouble, np.clongdouble
U = 2.0 ** -53
U_LD = float(np.finfo(LD).eps) / 2  # 2^-64 on x86-64
LN_MAX = 690.0  # |Re ln psi| up to which psi is a finite, normal double
with mpmath.workdps(30):
    PI_LD = LD(mpmath.nstr(+mpmath.pi, 25))


def make(kind: str, W, hb, vb=None) -> Rbm:
    """mcmc_replay.Rbm from float64 arrays; complex parameters as complex128 or as (re, im) pairs; vb None: no visible bias."""
    W, hb = np.asarray(W), np.asarray(hb)
    if kind == "complex":
        if not np.iscomplexobj(W):
            W = W[..., 0] + 1j * W[..., 1]
        if not np.iscomplexobj(hb):
            hb = hb[..., 0] + 1j * hb[..., 1]
        if vb is None:
            vb = np.zeros(W.shape[1], dtype=np.complex128)
        elif not np.iscomplexobj(vb):
            vb = np.asarray(vb)[..., 0] + 1j * np.asarray(vb)[..., 1]
        return Rbm(kind, W.astype(np.complex128), hb.astype(np.complex128), np.asarray(vb, dtype=np.complex128))
    vb = np.zeros(W.shape[1]) if vb is None else np.asarray(vb, dtype=np.float64)
    return Rbm(kind, W.astype(np.float64), hb.astype(np.float64), vb)


def pairs(z: np.ndarray) -> np.ndarray:
    """complex128 [...] -> float64 [..., 2], the kernels' (re, im) layout"""
    return np.ascontiguousarray(np.stack([z.real, z.imag], -1))


def mirrored(rbm: Rbm, units: np.ndarray) -> Rbm:
    """(W_h, b_h) -> (-W_h, -b_h) for the hidden units in `units`: psi is even in them (cosh is)."""
    W, hb = rbm.W.copy(), rbm.hb.copy()
    W[units], hb[units] = -W[units], -hb[units]
    return Rbm(rbm.kind, W, hb, rbm.vb)


def hidden_scale(rbm: Rbm) -> np.ndarray:
    """S_h = |b_h| + sum_o |W_ho| (longdouble [H])"""
    return np.abs(rbm.hb).astype(LD) + np.abs(rbm.W).astype(LD).sum(1)


@dataclass
class Exact:
    """ln psi of n rows.  re, im: Re / Im ln psi (im not wrapped; "tanh": the visible factor `vis` = tanh(a.x) is kept apart, re is ln of
    the hidden units' product; "pRBM": re = 0, im = a.x + sum ln 2cosh).  y: tanh theta [n, H].  cond: cond(x) [n]."""
    kind: str
    re: np.ndarray
    im: np.ndarray
    vis: np.ndarray
    cond: np.ndarray
    y: np.ndarray
    sech2: np.ndarray  # |1 - tanh^2 theta| [n, H]

    def psi(self) -> np.ndarray:
        """psi as clongdouble [n] (real flavours: zero imaginary part)"""
        m = np.exp(self.re) * self.vis
        return m * np.cos(self.im) + 1j * (m * np.sin(self.im))

    def im_principal(self) -> np.ndarray:
        """Im ln psi on (-pi, pi]"""
        return self.im - 2 * PI_LD * np.rint(self.im / (2 * PI_LD))


def exact_ld(rbm: Rbm, x: np.ndarray) -> Exact:
    """The reference in numpy longdouble for the +-1 rows x [n, sorb]."""
    assert rbm.kind in ("real", "tanh", "pRBM", "complex"), rbm.kind
    xl = x.astype(LD)
    if rbm.kind == "complex":
        a = rbm.hb.real.astype(LD) + xl @ rbm.W.real.T.astype(LD)
        b = rbm.hb.imag.astype(LD) + xl @ rbm.W.imag.T.astype(LD)
        return exact_from_theta(rbm, a, b, xl @ rbm.vb.real.astype(LD), xl @ rbm.vb.imag.astype(LD))
    return exact_from_theta(rbm, rbm.hb.astype(LD) + xl @ rbm.W.T.astype(LD), None, xl @ rbm.vb.astype(LD), None)


def exact_from_theta(rbm: Rbm, a: np.ndarray, b, axr: np.ndarray, axi) -> Exact:
    """exact_ld from theta = a + i b (longdouble [n, H]; b None for real parameters) and a.x = axr + i axi (longdouble [n]) of the rows:
    for callers that have theta of many rows which differ from one row in a few orbitals (eloc_exact)."""
    n = a.shape[0]
    S = hidden_scale(rbm)
    one, zero = np.ones(n, dtype=LD), np.zeros(n, dtype=LD)
    if rbm.kind == "complex":
        s = np.where(a < 0, LD(-1), LD(1))
        e = np.exp(-2 * np.abs(a))
        ome = -np.expm1(-2 * np.abs(a))  # 1 - e
        cb, sb = np.cos(b), np.sin(b)
        den = ome * ome + 4 * e * cb * cb
        with np.errstate(divide="ignore", invalid="ignore"):
            re = (np.abs(a) + 0.5 * np.log(den)).sum(1)
            im = (s * b + np.arctan2(-2 * s * e * sb * cb, ome + 2 * e * cb * cb)).sum(1)
            y = (s * ome * (1 + e) / den) + 1j * (4 * e * sb * cb / den)
        cond = 1 + (np.abs(y) * S).sum(1) + np.abs(rbm.vb).astype(LD).sum()
        return Exact(rbm.kind, re + axr, im + axi, one, cond.astype(np.float64), y, np.abs(1 - y * y).astype(np.float64))
    th, ax = a, axr
    e = np.exp(-2 * np.abs(th))
    lnh = (np.abs(th) + np.log1p(e)).sum(1)
    y = np.where(th < 0, LD(-1), LD(1)) * (-np.expm1(-2 * np.abs(th))) / (1 + e)
    cond = (1 + (np.abs(y) * S).sum(1) + np.abs(rbm.vb).astype(LD).sum()).astype(np.float64)
    sech2 = (4 * e / ((1 + e) * (1 + e))).astype(np.float64)
    if rbm.kind == "real":
        return Exact(rbm.kind, lnh + ax, zero, one, cond, y, sech2)
    if rbm.kind == "tanh":
        return Exact(rbm.kind, lnh, zero, np.tanh(ax), cond, y, sech2)
    return Exact(rbm.kind, zero, lnh + ax, one, cond, y, sech2)


_SHIFT = 1074  # every double is an integer multiple of 2^-1074


def _as_int(a: np.ndarray) -> np.ndarray:
    """float64 array -> object array of Python integers a * 2^1074 (exact)"""
    out = np.empty(a.shape, dtype=object)
    for idx, v in np.ndenumerate(a):
        num, den = float(v).as_integer_ratio()
        out[idx] = num * ((1 << _SHIFT) // den)
    return out


def exact_mp(rbm: Rbm, rows: np.ndarray, dps: int = MP_DPS + 10):
    """[(L, vis, cond)] of the +-1 rows [m, sorb] with mpmath at `dps` digits.  theta and a.x are summed EXACTLY (integer arithmetic on
    the doubles' mantissas) before they become mpmath numbers.  L = ln psi as an mpc with log's principal branch per hidden unit
    (compare the imaginary part modulo 2 pi), without the visible factor for "tanh" (vis = tanh(a.x), else 1); "pRBM":
    L = i (a.x + sum ln 2cosh)."""
    mp = mpmath.mp
    xi = np.asarray(rows).astype(np.int64).astype(object)
    cplx = rbm.kind == "complex"
    parts = (lambda z: (z.real, z.imag)) if cplx else (lambda z: (z,))
    th = [xi @ _as_int(np.ascontiguousarray(w)).T + _as_int(np.ascontiguousarray(b)) for w, b in zip(parts(rbm.W), parts(rbm.hb))]
    ax = [xi @ _as_int(np.ascontiguousarray(v)) for v in parts(rbm.vb)]
    out = []
    with mpmath.workdps(dps):
        one = mp.mpf(2) ** _SHIFT
        S = [mp.mpf(float(abs(b))) if not cplx else abs(mp.mpc(float(b.real), float(b.imag))) for b in rbm.hb]
        for h in range(rbm.H):
            S[h] += mp.fsum([abs(mp.mpc(float(w.real), float(w.imag))) if cplx else mp.mpf(float(abs(w))) for w in rbm.W[h]])
        sa = mp.fsum([abs(mp.mpc(float(v.real), float(v.imag))) if cplx else mp.mpf(float(abs(v))) for v in rbm.vb])
        for k in range(xi.shape[0]):
            tot, cond = mp.mpc(0), 1 + sa
            for h in range(rbm.H):
                t = mp.mpc(mp.mpf(int(th[0][k, h])) / one, mp.mpf(int(th[1][k, h])) / one) if cplx else mp.mpf(int(th[0][k, h])) / one
                tot += mp.log(2 * mp.cosh(t))
                cond += abs(mp.tanh(t)) * S[h]
            a = mp.mpc(mp.mpf(int(ax[0][k])) / one, mp.mpf(int(ax[1][k])) / one) if cplx else mp.mpf(int(ax[0][k])) / one
            if rbm.kind == "tanh":
                out.append((mp.mpc(tot), mp.tanh(a), cond))
            elif rbm.kind == "pRBM":
                out.append((mp.mpc(0, (tot + a).real), mp.mpf(1), cond))
            else:
                out.append((mp.mpc(tot + a), mp.mpf(1), cond))
    return out


def _mpf(v) -> mpmath.mpf:
    return mpmath.mpf(np.format_float_positional(v, unique=False, precision=25, trim="k")) if np.isfinite(v) else mpmath.mpf(str(v))


def check_against_mp(rbm: Rbm, x: np.ndarray, ex: Exact, rows) -> dict:
    """Compare the longdouble reference with mpmath on `rows`: asserts |ln psi_ld - ln psi_mp| (phase modulo 2 pi) and the visible factor
    within the amplitude bound's own derivation at longdouble's unit roundoff, U_LD (sorb + H + 16) cond(x), and cond to 1e-12 relative;
    returns the worst observed figures {"abs/cond", "rel", "cond_rel"}."""
    sorb = x.shape[1]
    worst = {"abs/cond": 0.0, "rel": 0.0, "cond_rel": 0.0}
    rows = np.asarray(rows, dtype=np.int64)
    for k, (L, vis, cond) in zip(rows, exact_mp(rbm, x[rows])):
        with mpmath.workdps(MP_DPS + 10):
            d = mpmath.mpc(_mpf(ex.re[k]), _mpf(ex.im[k])) - L
            d = mpmath.mpc(d.real, d.imag - 2 * mpmath.pi * mpmath.nint(d.imag / (2 * mpmath.pi)))
            err = float(abs(d))
            scale = float(abs(mpmath.mpc(_mpf(ex.re[k]), _mpf(ex.im[k]))))
            dv = float(abs(_mpf(ex.vis[k]) - vis))
            dc = float(abs(mpmath.mpf(float(ex.cond[k])) - cond) / cond)
        tol = U_LD * (sorb + rbm.H + 16) * float(cond)
        assert err <= tol and dv <= 4 * U_LD and dc <= 1e-12, (rbm.kind, int(k), err, tol, dv, dc)
        worst["abs/cond"] = max(worst["abs/cond"], err / float(cond))
        worst["rel"] = max(worst["rel"], err / max(scale, 1e-300))
        worst["cond_rel"] = max(worst["cond_rel"], dc)
    return worst


def exact(rbm: Rbm, x: np.ndarray, rng: np.random.Generator, nspot: int = 3) -> Exact:
    """exact_ld, checked against mpmath on every row when states x hidden units x orbitals <= MP_WORK, else on `nspot` random rows."""
    ex = exact_ld(rbm, x)
    n = x.shape[0]
    rows = np.arange(n) if n * rbm.H * x.shape[1] <= MP_WORK else rng.choice(n, size=min(nspot, n), replace=False)
    check_against_mp(rbm, x, ex, rows)
    return ex


def amp_bound(sorb: int, H: int, cond: np.ndarray) -> np.ndarray:
    """u (sorb + H + 16) cond(x): the bound on |psi / psi_exact - 1| (module docstring)"""
    return U * (sorb + H + 16) * np.asarray(cond, dtype=np.float64)


def amp_bound_exact_theta(rbm: Rbm) -> float:
    """The bound on |psi / psi_exact - 1| for the regime "exact-theta", where the generic bound's largest term -- the rounding of theta,
    (sorb + 1) u S_h with S_h >= |b_h| ~ 4000 -- does not exist: W = 0, so every fused multiply-add of the theta chain returns b_h
    unchanged; a.x is a sum of multiples of 2^-10 and exact; the phases s Im theta of a conjugate pair cancel exactly, so the final
    sine / cosine see an exact zero (children: sum_h Im theta_h likewise).  What is left, per hidden unit: the factor
    F_h = 1 + rho e^{-2 i s beta} with rho = exp(-2 |a|) <= 2 u relative, sine and cosine of 2 beta <= 3 u absolute (two roundings of the
    reduced argument, the polynomial; THE REDUCTION ITSELF MUST BE EXACT for that, which is what this regime is for: beta up to 4000 is
    2500 quarter turns), the two roundings that form F_h: |dF_h| <= 8 u, i.e. 8 u / |F_h| relative (the children's 1 + q_h, q_h = 1 / (rho
    e^{-2 i s beta}) or its inverse, has the same relative error); 3 u per complex multiplication of the running product; then the exponent
    Re a.x + sum_h |a_h| + e2 ln 2 (|e2| <= H) with H + 2 additions and the exponential's own u, and 4 u for the final products:
        u (16 + 3 H + 8 sum_h 1 / |F_h| + (H + 3) (1 + sum_o |a_o| + sum_h |a_h| + H ln 2))."""
    assert not rbm.W.any() and not rbm.vb.imag.any()
    a, beta = np.abs(rbm.hb.real).astype(LD), rbm.hb.imag.astype(LD)
    rho = np.exp(-2 * a)
    F = np.sqrt((1 - rho) ** 2 + 4 * rho * np.cos(beta) ** 2)
    H = rbm.H
    return U * float(16 + 3 * H + 8 * (1 / F).sum() + (H + 3) * (1 + np.abs(rbm.vb.real).sum() + a.sum() + H * np.log(2.0)))


def amp_ratio(rbm: Rbm, got: np.ndarray, ex: Exact) -> np.ndarray:
    """error / allowed error per row, float64 [n], from a kernel's psi (float64 or complex128 [n]) and the reference; inf where the
    kernel's value is not finite.  real, complex: |psi / psi_exact - 1| over amp_bound.  "pRBM": the phase difference and | |psi| - 1 |,
    absolute, over amp_bound.  "tanh": |psi - psi_exact| / prod_exact over amp_bound |tanh(a.x)| + u ((sorb + 1) sum_o |a_o| sech^2(a.x) + 1):
    the relative bound on everything but the visible factor, plus the absolute term of the visible factor's own argument and rounding
    (module docstring)."""
    sorb = rbm.W.shape[1]
    g = np.asarray(got)
    ok = np.isfinite(g.real) & np.isfinite(g.imag)
    gl = np.where(ok, g, 0).astype(CLD)
    ref = ex.psi()
    allowed = amp_bound(sorb, rbm.H, ex.cond)
    if rbm.kind == "pRBM":
        r = gl * np.conj(ref)  # |ref| = 1
        err = np.maximum(np.abs(np.arctan2(r.imag, r.real)), np.abs(np.abs(gl) - 1))
    elif rbm.kind == "tanh":
        err = np.abs(gl.real - ref.real) / np.exp(ex.re)
        vis = ex.vis.astype(np.float64)
        allowed = allowed * np.abs(vis) + U * ((sorb + 1) * float(np.abs(rbm.vb).sum()) * (1 - vis * vis) + 1)
    else:
        err = np.abs(gl / ref - 1)
    return np.where(ok, err.astype(np.float64) / allowed, np.inf)


@dataclass
class GradExact:
    """G_k and the loss in longdouble, the per-output bounds on |G_k - G_exact_k| (float64) and the bound on the loss."""
    GW: np.ndarray    # [H, sorb] (clongdouble for complex parameters, else longdouble: Re G)
    Ghb: np.ndarray   # [H]
    Gvb: np.ndarray   # [sorb]
    loss: float
    bW: np.ndarray    # [H, sorb]
    bhb: np.ndarray   # [H]
    bvb: np.ndarray   # [sorb]
    bloss: float
    sum_a: np.ndarray  # [H]: sum_n a_n |tanh theta_nh|  (the bound's first sum; visible bias: sum_a_vb)
    sum_f: np.ndarray  # [H]: sum_n |f_n| (...)         (the bound's second sum; visible bias: sum_f_vb)
    f: np.ndarray      # f_n


def grad_exact(rbm: Rbm, x: np.ndarray, prob: np.ndarray, eloc: np.ndarray, e_total, powc=None) -> GradExact:
    """The estimator of pynqs_rbm_grad in longdouble.  e_total: the SAME double(s) the kernel is given (an input, not recomputed)."""
    assert rbm.kind in ("real", "complex")
    n, sorb = x.shape
    H = rbm.H
    ex = exact_ld(rbm, x)
    cplx = rbm.kind == "complex"
    p = np.asarray(prob, dtype=np.float64).astype(LD)
    c = np.ones(n, dtype=LD) if powc is None else np.asarray(powc, dtype=np.float64).astype(LD)
    E = np.asarray(eloc).astype(CLD)
    Et = CLD(complex(e_total))
    f = p * (E - Et * c)
    fb = np.conj(f)
    xl = x.astype(LD)
    if cplx:
        GW = (fb[:, None] * ex.y).T @ xl.astype(CLD)
        Ghb = (fb[:, None] * ex.y).sum(0)
        Gvb = fb @ xl.astype(CLD)
    else:  # real parameters: only Re G enters the gradient, and O is real
        GW = (f.real[:, None] * ex.y).T @ xl
        Ghb = (f.real[:, None] * ex.y).sum(0)
        Gvb = f.real @ xl
    an = (p * (np.abs(E) + abs(Et) * np.abs(c))).astype(np.float64)
    af = np.abs(f).astype(np.float64)
    ay = np.abs(ex.y).astype(np.float64)
    S = hidden_scale(rbm).astype(np.float64)
    adds = 40 + n / 128
    sum_a = (an[:, None] * ay).sum(0)
    sum_f = (af[:, None] * (adds * np.maximum(1.0, ay) + (sorb + 2) * S[None, :] * ex.sech2)).sum(0)
    bhb = U * (4 * sum_a + sum_f)
    bW = np.repeat(bhb[:, None], sorb, 1)
    bvb = np.full(sorb, U * (4 * an.sum() + adds * af.sum()))
    lre, lim = ex.re, ex.im_principal()
    loss = 2 * (lre * f.real + lim * f.imag).sum()
    al = np.hypot(lre, lim).astype(np.float64)
    bloss = 2 * U * float((4 * an * al + af * (adds * np.maximum(1.0, al) + (sorb + H + 16) * ex.cond)).sum())
    return GradExact(GW, Ghb, Gvb, float(loss), bW, bhb, bvb, bloss, sum_a, sum_f, f)


def grad_errors(ge: GradExact, gw: np.ndarray, ghb: np.ndarray, gvb, cplx: bool):
    """(|G - G_exact| / bound) per output for the three parameter groups, from a kernel's gradient arrays (real parameters: float64 of
    the parameters' shapes, gradient = 2 Re G; complex: trailing [2] = (2 Re G, -2 Im G)).  Non-finite entries give inf."""
    out = []
    for g, ref, b in ((gw, ge.GW, ge.bW), (ghb, ge.Ghb, ge.bhb), (gvb, ge.Gvb, ge.bvb)):
        if g is None:
            out.append(np.zeros(0))
            continue
        g = np.asarray(g, dtype=np.float64)
        if cplx:
            ok = np.isfinite(g).all(-1)
            G = np.where(ok, g[..., 0], 0).astype(LD) / 2 - 1j * (np.where(ok, g[..., 1], 0).astype(LD) / 2)
        else:
            ok = np.isfinite(g)
            G = np.where(ok, g, 0).astype(LD) / 2
        assert G.shape == ref.shape == b.shape, (G.shape, ref.shape, b.shape)
        out.append(np.where(ok, np.abs(G - ref).astype(np.float64) / b, np.inf))
    return out


# ---- seeded inputs shared by the host tests (tests/test_rbm_exact.py) and the GPU tests (tests/test_gpu_rbm_exact.py) -----------------
REGIMES_ANY = ("small", "fe2s2", "alt30", "chunk+50", "chunk-50", "two-200", "one-338", "one-338-w", "spread-45", "novb")
REGIMES_ELOC = ("cross",)  # (tests/eloc_exact.py: excitations that take theta through zero)
REGIMES_COMPLEX = ("imb50", "imb1000", "exact-theta")
REGIMES_GRAD = ("tiny", "sat40")


def regime_params(regime: str, kind: str, sorb: int, H: int, seed: int) -> Rbm:
    """The parameter regimes of the exact tests.  small: all parameters 0.4 (U - 0.5); the others take W = w (U - 0.5), w = 0.2 min(1,
    40 / sorb) (so that sum_o |W_ho| stays near 2 for every sorb), b = U - 0.5, a = 0.2 (U - 0.5) -- "fe2s2" as it stands -- and then set
    Re b of some hidden units: alt30 +30 / -30 alternating on the first 16; chunk+50 / chunk-50 the whole first chunk of eight; two-200
    units 3 and 5 (one chunk) at -200; one-338 unit 3 at -338; one-338-w unit 3 with b = -346 and W = 4 on the four orbitals of
    forced_orbitals(sorb), else 0: theta = -330 exactly for a parent that occupies the four, -330 - 8 k with k of them flipped, so that
    four flips take exp(-2 theta) itself out of range (e^724) from a parent well inside it; spread-45 one unit per chunk of eight at -45 (at most 12); novb: small
    without a visible bias; imb50 (complex): Im b = 100 (U - 0.5); imb1000 (complex): six units with Im b = 2000 (U - 0.5) and Re b = +-2;
    exact-theta (complex, H even): W = 0, b in conjugate pairs a_j +- i beta_j with |a_j| in [0.2, 0.6] and beta_j in [500, 4000], a real
    and a multiple of 2^-10: theta_h = b_h, a.x and the sum of the phases carry NO rounding (see amp_bound_exact_theta);
    tiny: every parameter 1e-8 (U - 0.5); sat40: +40 / -40 alternating on the first 16 units; cross (H >= 3, sorb >= 4): fe2s2 with two
    hidden units, one of each sign of b, coupled by Re W = +-3 to the four orbitals of cross_orbitals(sorb) = (p0, p1, q0, q1), two of each
    spin: unit 1 has Re b = +1 and Re W = +3 / -3 on the alpha pair (p0, q0), unit 2 Re b = -1 and Re W = -3 / +3 on the beta pair (p1, q1).
    A row that occupies p0, p1 and leaves q0, q1 empty has theta = +7 / -7 (plus what the other orbitals add, about +-0.5); the excitation
    p -> q of that spin takes theta through zero to -5 / +5, where n_h prod q carries the factor and m_h does not; p -> elsewhere or
    elsewhere -> q stops at +-1.  (A unit coupled to all four would reach -+17, but then psi(x') / psi(x) spans e^-12 ... e^24 within one
    walker and a tenth of its columns lie below ANY rounding bound on E_loc, which is relative to the largest: each unit keeps to one spin,
    the ratios to [1e-5, 1], and every column stays visible -- tests/test_eloc_exact.py.)
    The numbers of biased units keep |Re ln psi| below LN_MAX."""
    g = np.random.default_rng([seed, sorb, H, len(regime)])
    cplx = kind == "complex"
    r = (lambda *s: (g.random(s) - 0.5) + 1j * (g.random(s) - 0.5)) if cplx else (lambda *s: g.random(s) - 0.5)
    if regime in ("small", "novb"):
        W, hb, vb = 0.4 * r(H, sorb), 0.4 * r(H), 0.4 * r(sorb)
        return make(kind, W, hb, None if regime == "novb" else vb)
    if regime == "tiny":
        return make(kind, 1e-8 * r(H, sorb), 1e-8 * r(H), 1e-8 * r(sorb))
    if regime == "exact-theta":
        assert cplx and H % 2 == 0
        a = np.where(g.random(H // 2) < 0.5, -1.0, 1.0) * (0.2 + 0.4 * g.random(H // 2))
        beta = 500.0 + 3500.0 * g.random(H // 2)
        hb = np.stack([a + 1j * beta, a - 1j * beta], 1).reshape(H)
        return make(kind, np.zeros((H, sorb), dtype=np.complex128), hb, np.round(0.2 * (g.random(sorb) - 0.5) * 1024) / 1024 + 0j)
    W, hb, vb = 0.2 * min(1.0, 40.0 / sorb) * r(H, sorb), r(H), 0.2 * r(sorb)

    def set_re(units, values):
        units = np.asarray(units)
        keep = units < H
        hb[units[keep]] = np.asarray(values, dtype=np.float64)[keep] + (1j * hb[units[keep]].imag if cplx else 0.0)

    if regime == "alt30":
        u = np.arange(16)
        set_re(u, np.where(u % 2 == 0, 30.0, -30.0) + g.random(16) - 0.5)
    elif regime == "chunk+50":
        set_re(np.arange(8), np.full(8, 50.0))
    elif regime == "chunk-50":
        set_re(np.arange(8), np.full(8, -50.0))
    elif regime == "two-200":
        set_re([3, 5] if H > 5 else [0, H - 1], [-200.0, -200.0])
    elif regime == "one-338":
        set_re([3 if H > 3 else 0], [-338.0])
    elif regime == "one-338-w":
        h3 = 3 if H > 3 else 0
        W[h3, :] = 0.0
        W[h3, forced_orbitals(sorb)] = 4.0
        set_re([h3], [-346.0])
    elif regime == "spread-45":
        u = np.arange(2 if H > 2 else 0, H, 8)[:12]
        set_re(u, np.full(u.size, -45.0))
    elif regime == "sat40":
        u = np.arange(16)
        set_re(u, np.where(u % 2 == 0, 40.0, -40.0) + g.random(16) - 0.5)
    elif regime == "cross":
        assert H >= 3 and sorb >= 4
        p0, p1, q0, q1 = cross_orbitals(sorb)
        for h, p, q, sg in ((1, p0, q0, 1.0), (2, p1, q1, -1.0)):
            W[h, p] = 3.0 * sg + (1j * W[h, p].imag if cplx else 0.0)
            W[h, q] = -3.0 * sg + (1j * W[h, q].imag if cplx else 0.0)
        set_re([1, 2], [1.0, -1.0])
    elif regime == "imb50":
        assert cplx
        hb = hb.real + 100j * (g.random(H) - 0.5)
    elif regime == "imb1000":
        assert cplx
        k = min(H, 6)
        hb[:k] = np.where(g.random(k) < 0.5, -2.0, 2.0) + 2000j * (g.random(k) - 0.5)
    else:
        assert regime == "fe2s2", regime
    return make(kind, W, hb, vb)


def forced_orbitals(sorb: int):
    """the four orbitals the regime "one-338-w" couples to its saturated unit: the word edges that exist, filled up from orbital 1 on"""
    f = sorted({o for o in (0, 63, 64, 127, 128, sorb - 1) if o < sorb})[:4]
    o = 1
    while len(f) < 4:
        if o not in f:
            f.append(o)
        o += 1
    return sorted(f)


def cross_orbitals(sorb: int):
    """(p0, p1, q0, q1) of the regime "cross": p0, q0 alpha (even) and p1, q1 beta (odd) orbitals, at the word edges that exist (0, 64,
    128; 63, 127, the last orbital), filled up with the lowest ones"""
    assert sorb >= 4
    alpha = [o for o in (0, 64, 128) if o < sorb]
    beta = [o for o in (63, 127, sorb - 1 if sorb & 1 == 0 else sorb - 2) if 0 < o < sorb]
    alpha = (alpha + [o for o in range(2, sorb, 2) if o not in alpha])[:2]
    beta = (beta + [o for o in range(1, sorb, 2) if o not in beta])[:2]
    return alpha[0], beta[0], alpha[1], beta[1]


def rand_words(n: int, sorb: int, seed: int, fill: float = 0.4) -> np.ndarray:
    """n random determinants as uint64 [n, len] words (orbital o = bit o; the bits above sorb are zero)"""
    g = np.random.default_rng([seed, n, sorb])
    return pack_bits(g.random((n, sorb)) < fill)


def pack_bits(bits: np.ndarray) -> np.ndarray:
    n, sorb = bits.shape
    L = (sorb - 1) // 64 + 1
    full = np.zeros((n, 64 * L), dtype=np.uint8)
    full[:, :sorb] = bits
    return np.ascontiguousarray(np.packbits(full, axis=1, bitorder="little")).view(np.uint64).reshape(n, L)


def flipped(words: np.ndarray, orbitals) -> np.ndarray:
    """one row of words with the given orbitals flipped"""
    out = words.copy()
    for o in orbitals:
        out[o >> 6] ^= np.uint64(1) << np.uint64(o & 63)
    return out


def make_children(parents: np.ndarray, sorb: int, seed: int, force=None):
    """Children of every parent row, built on the host so that every structure of pynqs_rbm_forward_children is hit on purpose:
    the parent itself (no flip), 2 and 4 random flips, flips at the word edges (orbitals 0, 63, 64, 127, 128, sorb - 1 where they exist,
    in pairs and four at once), four flips inside one word, four flips spread over all the words; several children per parent, and the
    list shuffled so that the parents come out of order; `force` (orbitals): also the first two and all of these flipped.  Returns (children uint64 [m, len], parent int32 [m], number of flips [m])."""
    g = np.random.default_rng([seed, sorb, parents.shape[0]])
    L = parents.shape[1]
    edges = sorted({o for o in (0, 63, 64, 127, 128, sorb - 1) if o < sorb})
    rows, par = [], []
    for p, w in enumerate(parents):
        sets = [[], list(g.choice(sorb, 2, replace=False)), list(g.choice(sorb, min(4, sorb), replace=False))]
        sets += [edges[i:i + 2] for i in range(0, len(edges), 2)] + [edges[:4], edges[-4:]]
        word = int(g.integers(L))
        lo, hi = 64 * word, min(64 * word + 64, sorb)
        if hi - lo >= 4:
            sets.append(list(lo + g.choice(hi - lo, 4, replace=False)))
        spread = [int(64 * k + g.integers(min(64, sorb - 64 * k))) for k in range(L)]
        while len(spread) < min(4, sorb):
            o = int(g.integers(sorb))
            if o not in spread:
                spread.append(o)
        sets.append(spread)
        if force is not None:
            sets += [list(force[:2]), list(force)]
        for s in sets:
            rows.append(flipped(w, [int(o) for o in s]))
            par.append(p)
    rows, par = np.stack(rows), np.asarray(par, dtype=np.int32)
    order = g.permutation(len(par))
    rows, par = rows[order], par[order]
    nflip = np.unpackbits((rows ^ parents[par]).view(np.uint8), axis=1).sum(1)
    assert nflip.max() <= 4
    return np.ascontiguousarray(rows), par, nflip


def children_form(sorb: int, H: int, kind: str) -> str:
    """"lds" / "wave": which form pynqs_rbm_forward_children takes, from the size of the factor table (include/pynqs_amd.h):
    (2 sorb + 1) ((H + 2) | 1) entries of 8 bytes (16 for complex parameters), in LDS up to 64 KB."""
    return "lds" if (2 * sorb + 1) * ((H + 2) | 1) * (16 if kind == "complex" else 8) <= 64 * 1024 else "wave"


def checked_case(kind: str, sorb: int, H: int, regime: str, words: np.ndarray, seed: int = 0, nspot: int = 2, rbm=None):
    """(rbm, x, Exact) of a case with the conditions that keep a comparison from passing vacuously asserted on the reference alone: every
    row's psi is a finite normal double (|Re ln psi| <= LN_MAX), no row is left out, and for complex parameters max cond(x) <= 1e4.
    rbm: the regime's parameters with a caller's changes (tests/children_cases.py), else regime_params(regime, ...)."""
    if rbm is None:
        rbm = regime_params(regime, kind, sorb, H, seed)
    assert rbm.kind == kind and rbm.W.shape == (H, sorb)
    x = pm1(words, sorb)
    ex = exact(rbm, x, np.random.default_rng(seed), nspot)
    assert x.shape[0] == words.shape[0] and np.isfinite(ex.cond).all()
    assert float(np.abs(ex.re).max()) <= LN_MAX, (kind, regime, float(np.abs(ex.re).max()))
    if kind == "complex" and regime != "exact-theta":  # (exact-theta: cond is |b| ~ 4000 per unit by design, and its bound does not use it)
        assert float(ex.cond.max()) <= 1e4, (regime, float(ex.cond.max()))
    if kind == "tanh":
        assert bool((ex.vis != 0).all())
    return rbm, x, ex
