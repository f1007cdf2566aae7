"""Plain numpy / float64 statements of what the train-mode BatchNorm entries of csrc/train_ops.hip promise, each in terms of the inputs
the entry is given (mean, invstd, `out` and the mask bytes are inputs, never recomputed), with a per-element error bound beside every
value.  Imports nothing of the package: tests/test_gpu_bn_entries.py holds the kernels to it, tests/test_bn_oracle_host.py holds it to
float64 torch.autograd.

Error bounds.  EPS = 2^-24 is the unit roundoff of float32.  A bound is k * EPS * (sum of the absolute values of the expression's
terms), k = (float32 roundings on the path to that term) + 1; the count stands in a comment beside each expression.  Layout: activations
are NHWC arrays (N, H, W, C); per-channel vectors broadcast along the last axis."""
import numpy as np

EPS = 2.0 ** -24
TR_BLOCKS, TR_APPLY_THREADS, TR_APPLY_BLOCKS, TR_EW, TR_UNROLL = 512, 1024, 512, 4, 8
P2_ROW, P2_INV_SLOT = 512, 511
F64_SUM = 2.0 ** -43  # relative error of a float64 sum of the kernels' partial chains (<= ~600 sequential terms of 2^-53 each)


def f64(a):
    return np.asarray(a, dtype=np.float64)


# ---- the P2 format (conv_p2.h) ---------------------------------------------------------------------------------------------------
def p2_scale(bound):
    """p2_scale_of: the exponent s that puts `bound` in [2^13, 2^14), from the float32 bits; e of 0 or 255 gives s = 0."""
    e = (int(np.float32(bound).view(np.uint32)) >> 23) & 0xFF
    s = 0 if e in (0, 255) else 13 - (e - 127)
    return max(-110, min(110, s))


def p2_inv_bits(s):
    """The dword a row's slot 511 holds: the float32 bits of 2^-s."""
    return (127 - s) << 23


def p2_encode(x_nhwc, s):
    """fp16 halves [n][plane h, l][C / 8][H][W][8]: h = fp16(x * 2^s), l = fp16(x * 2^s - h) (x * 2^s and the difference are exact in float32)."""
    x = np.asarray(x_nhwc, dtype=np.float32)
    n, h, w, c = x.shape
    assert c % 8 == 0
    v = x * np.float32(2.0 ** s)
    hi = v.astype(np.float16)
    lo = (v - hi.astype(np.float32)).astype(np.float16)
    g = lambda a: a.reshape(n, h, w, c // 8, 8).transpose(0, 3, 1, 2, 4)
    return np.ascontiguousarray(np.stack([g(hi), g(lo)], axis=1))


def p2_planes(halves, n, c, h, w):
    """(h, l) as float64 NHWC arrays."""
    a = np.asarray(halves).reshape(n, 2, c // 8, h, w, 8).astype(np.float64)
    g = lambda p: p.transpose(0, 2, 3, 1, 4).reshape(n, h, w, c)
    return g(a[:, 0]), g(a[:, 1])


def p2_decode(halves, inv, n, c, h, w):
    hi, lo = p2_planes(halves, n, c, h, w)
    return (hi + lo) * float(inv)


def p2_format_bound(x, inv):
    """The format's own statement: 22 bits above 2^-3 scaled, else 2^-25 * inv absolute."""
    return 2.0 ** -22 * np.abs(f64(x)) + 2.0 ** -25 * float(inv)


def wave_map(c):
    """p2_wave_map: (CB, CQ, PXW, NCB)."""
    cb = 32 if c % 32 == 0 else 16 if c % 16 == 0 else 8
    cq = cb // 4
    return cb, cq, 64 // cq, c // cb


# ---- the launchers' arithmetic ---------------------------------------------------------------------------------------------------
def _ceil(a, b):
    return -(-a // b)


def launch_geometry(kind, c, m, mo=None):
    """What the launcher of `kind` makes of C channels, M conv-resolution pixels and (apply kinds) Mo output pixels.
    kinds: 'stats' (bn_stats_partial_kernel: TR_UNROLL pixels per thread and trip), 'reduce' (the backward reductions at up == 0: TR_EW),
    'reduce_up' (bn_bwd_reduce_kernel at up > 0: one pixel), 'scalar' (bias_bwd_scalar_kernel), 'apply' (the float4 streams),
    'apply_p2' (the wave-per-(pixel chunk, channel block) streams), 'plane_stats'.
    trips = passes of the longest-running thread's loop; ragged = the last pass (or batch) is not full."""
    mo = m if mo is None else mo
    if kind in ("stats", "reduce", "reduce_up"):
        c4 = c // 4
        lanes = min(c4, 256)
        rows = 256 // lanes
        nb = min(TR_BLOCKS, _ceil(m, rows))
        per = {"stats": TR_UNROLL, "reduce": TR_EW, "reduce_up": 1}[kind] * nb * rows
        passes = _ceil(c4, lanes)
        return dict(nb=nb, lanes=lanes, rows=rows, idle=256 - lanes * rows, trips=_ceil(m, per), ragged=m % per != 0, cb_passes=passes,
                    cb_last=c4 - (passes - 1) * lanes)
    if kind == "scalar":
        rows = 256 // c
        nb = min(TR_BLOCKS, _ceil(m, rows))
        return dict(nb=nb, rows=rows, idle=256 - rows * c, trips=_ceil(m, nb * rows), ragged=m % (nb * rows) != 0)
    if kind == "apply":
        total = mo * (c // 4)
        nb = min(TR_APPLY_BLOCKS, _ceil(total, TR_APPLY_THREADS))
        return dict(nb=nb, trips=_ceil(total, nb * TR_APPLY_THREADS), ragged=total % (nb * TR_APPLY_THREADS) != 0)
    if kind == "apply_p2":
        _, _, pxw, ncb = wave_map(c)
        nb = min(TR_APPLY_BLOCKS, _ceil(mo * (c // 4), TR_APPLY_THREADS))
        nwork, nwaves = _ceil(mo, pxw) * ncb, nb * (TR_APPLY_THREADS // 64)
        return dict(nb=nb, trips=_ceil(nwork, nwaves), ragged=nwork % nwaves != 0 or mo % pxw != 0, partial_chunk=mo % pxw != 0)
    if kind == "plane_stats":
        total = mo * (c // 8)
        nb = min(1024, _ceil(total, 256))
        return dict(nb=nb, trips=_ceil(total, nb * 256), ragged=total % (nb * 256) != 0)
    raise ValueError(kind)


# ---- batch statistics ------------------------------------------------------------------------------------------------------------
def batch_stats(z, eps, momentum=None, running_mean=None, running_var=None):
    """mval_bn_batch_stats / mval_bn_finalize_stats: mean, biased invstd (and the running statistics with the unbiased variance), each
    (value, bound).  The device sums z and z^2 in float64 and takes var = E[z^2] - mean^2: the cancellation is charged at F64_SUM."""
    z = f64(z).reshape(-1, np.shape(z)[-1])
    m = z.shape[0]
    mu = z.mean(0)
    var = ((z - mu) ** 2).mean(0)
    ez2 = (z ** 2).mean(0)
    eps = float(np.float32(eps))
    r = {}
    r["mean"] = (mu, 2 * EPS * np.abs(mu) + F64_SUM * np.abs(z).mean(0))  # 1 rounding: the cast of the float64 mean
    istd = 1.0 / np.sqrt(var + eps)
    cancel = F64_SUM * 2.0 * ez2  # of var: both E[z^2] and mean^2
    r["invstd"] = (istd, 2 * EPS * istd + 0.5 * istd * cancel / (var + eps))  # 1 rounding: the cast
    if running_mean is not None:
        mom = float(np.float32(momentum))
        one_m = float(np.float32(1.0) - np.float32(momentum))
        rm, rv = f64(running_mean), f64(running_var)
        unb = var * m / (m - 1) if m > 1 else var
        # 5 roundings: (1 - m), (1 - m) * running, the cast of the statistic, m * stat, the sum
        r["running_mean"] = (one_m * rm + mom * mu, 6 * EPS * (np.abs(one_m * rm) + np.abs(mom * mu)) + mom * r["mean"][1])
        r["running_var"] = (one_m * rv + mom * unb, 6 * EPS * (np.abs(one_m * rv) + np.abs(mom * unb)) + mom * cancel * (m / max(m - 1, 1)))
    return r


# ---- forward ---------------------------------------------------------------------------------------------------------------------
def upsample(a, up):
    rep = 1 << up
    return a if up == 0 else np.repeat(np.repeat(a, rep, axis=1), rep, axis=2)


def window_sum(a, up):
    rep = 1 << up
    n, ho, wo, c = a.shape
    return a if up == 0 else a.reshape(n, ho // rep, rep, wo // rep, rep, c).sum(axis=(2, 4))


def bn_forward(z, mean, invstd, gamma, beta, up=0, relu=False, r1=None, r2=None, stat_err=False):
    """out = act(((z * alpha + (beta - mean * alpha)) up) + r1 + r2), alpha = invstd * gamma.  Returns dict(out, bound, pre, mag):
    pre = the pre-activation, mag = the sum of its terms' magnitudes.  Asserts that no element's ReLU mask is undecided:
    min |pre| >= 2^-10 * mag (the bound is below 2^-21 * mag).  stat_err: mean and invstd are the float64 statistics the device only has
    rounded to float32 -- two roundings more."""
    z, mean, invstd, gamma, beta = f64(z), f64(mean), f64(invstd), f64(gamma), f64(beta)
    alpha = invstd * gamma
    y = upsample(z * alpha + (beta - mean * alpha), up)
    mag = upsample(np.abs(z * alpha) + np.abs(mean * alpha) + np.abs(beta), up) + np.zeros_like(y)
    k = 3  # alpha = invstd * gamma, beta' = fma(-mean, alpha, beta), fma(z, alpha, beta')
    pre = y
    for r in (r1, r2):
        if r is not None:
            pre = pre + f64(r)
            mag = mag + np.abs(f64(r))
            k += 1  # one float32 add per residual
    if stat_err:
        k += 2
    bound = (k + 1) * EPS * mag
    if relu:
        assert (np.abs(pre) >= 2.0 ** -10 * mag).all(), "undecided ReLU mask: min |pre| / mag = %.3g" % float((np.abs(pre) / mag).min())
    return dict(out=np.maximum(pre, 0.0) if relu else pre, bound=bound, pre=pre, mag=mag)


def fwd_bound(gamma, beta, m, r1max=0.0, r2max=0.0):
    """The a-priori bound the P2 forward apply scales by: Samuelson's |xhat| <= sqrt(M - 1) plus the residuals' exact maxima."""
    return float((np.abs(f64(gamma)) * np.sqrt(max(m - 1.0, 1.0)) + np.abs(f64(beta))).max() * (1 + 1e-6) + r1max + r2max)


def mask_bits(out):
    """One byte per float4 of `out`: bit k = (out[4 q + k] > 0)."""
    o = (np.asarray(out).reshape(-1, 4) > 0).astype(np.uint8)
    return o[:, 0] | (o[:, 1] << 1) | (o[:, 2] << 2) | (o[:, 3] << 3)


# ---- backward --------------------------------------------------------------------------------------------------------------------
def masked_gradient(gout, mode, out=None, bits=None, z=None, mean=None, invstd=None, gamma=None, beta=None):
    """gout where the ReLU let the activation through.  mode 0: no mask, 1: out > 0, 2: bn_affine(z) > 0 (the decided-mask condition is
    asserted on z), 3: the kept bits (one byte per float4)."""
    g = f64(gout)
    if mode == 0:
        return g
    if mode == 1:
        keep = np.asarray(out) > 0
    elif mode == 2:
        keep = bn_forward(z, mean, invstd, gamma, beta, relu=True)["pre"] > 0
    else:
        b = np.asarray(bits, dtype=np.uint8).reshape(-1, 1)
        keep = ((b >> np.arange(4, dtype=np.uint8)) & 1).astype(bool).reshape(g.shape)
    return np.where(keep, g, 0.0)


def residual_gradient(g, prior, store):
    """A residual's gradient slot after the call: the masked gradient stored (exact) or added to `prior` (1 rounding)."""
    if store:
        return g, np.zeros_like(g)
    return f64(prior) + g, 2 * EPS * (np.abs(f64(prior)) + np.abs(g))


def bn_backward(g, z, mean, invstd, gamma, up=0, has_bn=True, stat_err=False):
    """g: the masked gradient at the OUTPUT resolution (float32 values).  Returns dict of (value, bound) pairs: gz (the window sum over
    the 2^up x 2^up replicas), dbeta, and with has_bn dgamma and dz = gamma * invstd * (gz - dbeta / M - xhat * dgamma / M)."""
    g = f64(g)
    rep2 = (1 << up) ** 2
    gz = window_sum(g, up)
    e_g = (rep2 - 1) * EPS * window_sum(np.abs(g), up)  # rep^2 - 1 float32 adds (0 + g is exact), each below EPS * sum |g|
    c = g.shape[-1]
    m = gz.size // c
    ax = (0, 1, 2)
    r = {"gz": (gz, e_g)}
    db = gz.sum(ax)
    e_db = e_g.sum(ax) + EPS * np.abs(gz).sum(ax) + EPS * np.abs(db)  # float64 sum of float32 values; 1 rounding: the cast
    r["dbeta"] = (db, e_db)
    if not has_bn:
        return r
    z, mean, invstd, gamma = f64(z), f64(mean), f64(invstd), f64(gamma)
    xh = (z - mean) * invstd
    e_x = np.abs(mean) * invstd * EPS + np.abs(xh) * EPS if stat_err else 0.0  # (mean and invstd only known to float32)
    dg = (gz * xh).sum(ax)
    # xhat in float32: z - mean, * invstd (2 roundings), products and sum in float64; 1 rounding: the cast
    e_dg = (e_g * np.abs(xh)).sum(ax) + 3 * EPS * np.abs(gz * xh).sum(ax) + EPS * np.abs(dg) + (np.abs(gz) * e_x).sum(ax)
    r["dgamma"] = (dg, e_dg)
    a = np.abs(gamma * invstd)
    dz = gamma * invstd * (gz - db / m - xh * dg / m)
    # r = (gamma * invstd) * (g - db * invM - xh * (dg * invM)), invM = 1 / (float)M, train_ops.hip bn_bwd_apply*_kernel.  Roundings on the
    # path of the term with most: xh * dg / M -- z - mean, * invstd, the cast of dgamma, invM, dg * invM, xh * (...), the subtraction,
    # gamma * invstd, the final product = 9 (db / M: 7, g: 4).  The sums' own errors enter through db / M and xh * dg / M.
    terms = np.abs(gz) + np.abs(db) / m + np.abs(xh * dg) / m
    e_dz = a * (10 * EPS * terms + e_g + e_db / m + np.abs(xh) * e_dg / m + e_x * np.abs(dg) / m) + (EPS * np.abs(dz) if stat_err else 0.0)
    r["dz"] = (dz, e_dz)
    r["xhat"] = xh
    return r


def bwd_bound(gamma, invstd, gmax, dbeta, dgamma, m):
    """The a-priori bound of |dz| bn_bwd_finalize_bound_kernel leaves in *bound_slot."""
    a = np.abs(f64(gamma) * f64(invstd))
    return float((a * (gmax + np.abs(f64(dbeta)) / m + np.sqrt(max(m - 1.0, 1.0)) * np.abs(f64(dgamma)) / m)).max() * (1 + 1e-5))


def far_from_power_of_two(bound):
    """The exponent p2_scale reads is unambiguous: `bound` is not within 1e-4 relative of a power of two."""
    mant = bound / 2.0 ** np.floor(np.log2(bound))  # in [1, 2)
    return mant > 1.0 + 1e-4 and mant < 2.0 * (1.0 - 1e-4)
