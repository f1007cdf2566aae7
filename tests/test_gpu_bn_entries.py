"""The train-mode BatchNorm entries of csrc/train_ops.hip, each called alone through ctypes and held to the float64 statements of
tests/bn_oracle.py: batch statistics and both finalizers, the forward apply (fp32 and P2 forms, residuals as fp32 or as planes), the
plane statistics, the backward pair and its fused forms (fp32 and P2), the scalar bias form, one chain per mask mode, and the argument
checks that return before any launch.

Every output lives between two guards of 256 dwords inside one allocation, all prefilled with a NaN pattern: after a launch the guards
must be unchanged and every documented element written.  Buffer sizes are those of the header comments (ws 512 * C * 2 doubles, rows
576 dwords, P2 rows N * 512 dwords).  Tolerances are the oracle's own (k * 2^-24 * sum of term magnitudes, counted there); each test
prints its worst error / bound ratio.  The case tables below are held to the launchers' arithmetic by tests/test_bn_oracle_host.py
(no GPU), which also asserts the conditions on the inputs (decided ReLU masks, P2 bounds away from powers of two)."""
import ctypes as C

import numpy as np
import pytest
import torch

import bn_oracle as bo

gpu = pytest.mark.gpu

ROW = 576  # dwords of a training magnitude row: [count, <= 512 partial maxima] (engine_train.TRAIN_AMAX_ROW)
GUARD = 256  # dwords on either side of every output
SENT = 0x7FA57FA5  # a NaN as float32, a NaN in either fp16 half, every byte above 15: nothing a kernel stores
BN_EPS = 1e-5
_TORCH = {np.float32: torch.float32, np.float64: torch.float64, np.int32: torch.int32, np.uint8: torch.uint8, np.float16: torch.float16}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    from multi_view_active_learning_amd import _lib

    _lib.lib()
    return torch.device("cuda:0")


# ---- case tables (shapes are (n, h, w, c) at the conv resolution) -----------------------------------------------------------------
TWO_TRIP_STATS = (2, 257, 256, 32)  # M = 131584 > 8 * 512 * 32: the stats kernel's second trip, ragged
TWO_TRIP_APPLY = (2, 184, 180, 32)  # 2119680 outputs > 512 * 1024 float4 (and 8280 > 8192 wave items of the P2 kernels)
TWO_TRIP_REDUCE = (2, 129, 256, 32)  # M = 66048 > 4 * 512 * 32: the reductions' second TR_EW trip (8256 > 8192 wave items)

STATS_CASES = [(3, 5, 3, 4), (2, 7, 5, 16), (3, 5, 7, 48), (1, 3, 4, 1032), (1, 3, 4, 2048), TWO_TRIP_STATS]
TILES_CASE = (2, 30, 25, 8, 300)  # (n, h, w, c, tiles): more than the finalizer's 256 threads

# (n, h, w, c, up, relu, (kind of res1, kind of res2)); kinds: "none", "f32", "p2"
FWD_CASES = [
    (3, 5, 3, 4, 0, 1, ("none", "none")),
    (2, 7, 5, 16, 1, 1, ("f32", "none")),
    (3, 5, 3, 48, 2, 0, ("f32", "f32")),
    (1, 3, 4, 1032, 0, 1, ("none", "f32")),
    (2, 3, 3, 16, 2, 1, ("none", "none")),
    (2, 4, 3, 48, 1, 1, ("f32", "f32")),
    (3, 5, 3, 16, 0, 0, ("f32", "f32")),
    TWO_TRIP_APPLY + (0, 1, ("f32", "none")),
]
FWD_P2_CASES = [
    (3, 5, 3, 32, 0, 1, ("none", "none")),
    (3, 5, 3, 64, 0, 1, ("f32", "p2")),
    (3, 5, 3, 48, 0, 1, ("p2", "f32")),
    (2, 5, 3, 16, 1, 0, ("p2", "p2")),
    (3, 5, 3, 24, 2, 1, ("f32", "none")),
    (3, 5, 3, 8, 0, 1, ("none", "p2")),
    (1, 7, 9, 32, 1, 1, ("none", "f32")),
    (3, 5, 3, 64, 0, 0, ("p2", "none")),
    TWO_TRIP_APPLY + (0, 1, ("p2", "f32")),
]
PLANE_STATS_CASES = [FWD_P2_CASES[0], FWD_P2_CASES[2], FWD_P2_CASES[4], FWD_P2_CASES[8]]

# (n, h, w, c, up, relu, has_bn, (gres1 given, gres2 given), overwrite) of mval_bn_bwd / mval_bn_bwd_amax
BWD_CASES = [
    (3, 5, 3, 4, 0, 1, 1, (1, 1), 0),
    (2, 7, 5, 16, 0, 0, 1, (1, 1), 1),
    (3, 5, 3, 48, 0, 1, 1, (1, 1), 2),
    (1, 3, 4, 1032, 0, 1, 1, (1, 1), 3),
    (1, 3, 4, 2048, 0, 0, 1, (0, 0), 0),
    (2, 4, 3, 16, 1, 0, 1, (1, 1), 1),  # the no-ReLU four-at-a-time path: one round of 4,
    (2, 3, 2, 48, 2, 0, 1, (1, 1), 2),  # four rounds,
    (1, 3, 2, 16, 3, 0, 1, (1, 1), 0),  # sixteen
    (1, 3, 2, 16, 3, 0, 1, (0, 1), 3),
    (2, 4, 3, 16, 1, 1, 1, (1, 0), 3),
    (2, 3, 2, 16, 2, 1, 1, (1, 1), 1),
    (1, 2, 2, 4, 3, 1, 1, (1, 1), 2),
    (3, 5, 3, 16, 0, 1, 0, (1, 1), 2),  # has_bn = 0: the conv + bias layers
    (2, 4, 3, 48, 1, 0, 0, (1, 0), 0),
    TWO_TRIP_REDUCE + (0, 1, 1, (1, 0), 0),
    (2, 130, 128, 16, 1, 0, 1, (1, 0), 0),  # M = 33280 > 512 * 64: the up-sampled loop's second trip
]
# (n, h, w, c, relu) of the scalar form (C % 4 != 0); M = 7000 is more than 512 workgroups' rows at C = 19 (13 rows each)
SCALAR_CASES = [(2, 5, 3, 19, 1), (2, 5, 3, 19, 0), (2, 5, 3, 17, 1), (2, 5, 3, 17, 0), (3, 7, 5, 1, 1), (3, 7, 5, 1, 0), (1, 70, 100, 19, 1)]

# (n, h, w, c, mask mode, (gres1 given, gres2 given), overwrite) of mval_bn_bwd_fused / _fused_mask.  Mode 0: no ReLU; 1: ReLU with
# residuals, mask from `out`; 2: ReLU without residuals, mask from z; 3: ReLU with residuals, mask from the kept bytes.
FUSED_CASES = [
    (3, 5, 3, 4, 0, (1, 1), 0),
    (2, 7, 5, 16, 0, (0, 0), 0),
    (3, 5, 3, 48, 1, (1, 1), 1),
    (2, 7, 5, 16, 1, (1, 1), 2),
    (2, 7, 5, 16, 1, (0, 1), 3),
    (1, 3, 4, 1032, 2, (0, 0), 0),
    (1, 3, 4, 2048, 2, (0, 0), 0),
    (3, 5, 3, 48, 3, (1, 1), 3),
    (2, 7, 5, 16, 3, (1, 0), 0),
    (3, 5, 3, 4, 3, (1, 1), 2),
    TWO_TRIP_REDUCE + (1, (1, 1), 1),
    # no given slot is stored: the apply pass re-reads gout and derives the mask again (apply_mask below) from `out` ...
    (3, 5, 3, 48, 1, (1, 1), 0),
    (2, 7, 5, 16, 1, (1, 0), 2),
    TWO_TRIP_REDUCE + (1, (1, 1), 0),
    # ... or from the kept bytes
    (3, 5, 3, 48, 3, (1, 1), 0),
    TWO_TRIP_REDUCE + (3, (0, 1), 1),
    TWO_TRIP_REDUCE + (2, (0, 0), 0),
]
BWD_P2_CASES = [
    (3, 5, 3, 32, 0, (1, 1), 1),
    (3, 5, 3, 24, 0, (0, 0), 0),
    (3, 5, 3, 48, 1, (1, 1), 2),
    (3, 5, 3, 24, 2, (0, 0), 0),
    (2, 7, 5, 48, 2, (0, 0), 0),
    (3, 5, 3, 32, 3, (1, 1), 0),
    (3, 5, 3, 48, 3, (0, 1), 2),
    TWO_TRIP_REDUCE + (3, (1, 0), 1),
    # no given slot is stored: the apply pass masks gout itself, from `out` (bn_bwd_apply2_p2_kernel<1>) ...
    (3, 5, 3, 48, 1, (1, 1), 0),
    (2, 7, 5, 24, 1, (1, 0), 2),
    TWO_TRIP_REDUCE + (1, (0, 1), 1),
    # ... or from the kept bytes (<3>)
    (3, 5, 3, 24, 3, (0, 1), 1),
    TWO_TRIP_REDUCE + (3, (1, 1), 0),
    TWO_TRIP_REDUCE + (2, (0, 0), 0),
]
CHAIN_OVERWRITE = {0: 3, 1: 0, 2: 0, 3: 0}  # by mask mode: the ReLU ops with residuals accumulate, so their apply pass masks gout itself
CHAIN_CASES = [(3, 5, 3, 32, 0), (3, 5, 3, 48, 1), (3, 5, 3, 24, 2), (3, 5, 3, 64, 3)]  # (n, h, w, c, mask mode)


def apply_mask(mode, slots, overwrite):
    """The mask mode the APPLY pass of mval_bn_bwd_fused_p2 runs with: a given slot the call stores holds the masked gradient already, and
    the pass re-reads that slot unmasked; otherwise it re-reads gout and masks it as the reduction did."""
    return 0 if (slots[0] and overwrite & 1) or (slots[1] and overwrite & 2) else mode


def _id(case):
    return "-".join("".join(str(int(v)) if not isinstance(v, str) else v[0] for v in x) if isinstance(x, tuple) else str(x) for x in case)


# ---- inputs, by construction (numpy only: the host file builds the same data) -----------------------------------------------------
def _seed(case):
    return sum((i + 1) * 7919 * (hash(x) % 1000003 if not isinstance(x, (tuple, str)) else len(str(x))) for i, x in enumerate(case)) % (2 ** 31)


def make_case(n, h, w, c, up=0, relu=1, kinds=("none", "none"), seed=0, offset=1.0):
    """Inputs of one forward (and of the backward behind it) whose every ReLU mask is decided: the wanted pre-activation r is drawn with
    |r| >= 0.25 (>= the 0.05 floor), z is solved from it, z = (r - beta - res) / alpha + mean, and rounded to float32; mean and invstd are
    then the TRUE statistics of that float32 z (float64, rounded), gamma and beta re-solved for them -- so Samuelson's bound holds for
    the data and bn_forward's assertion re-checks the condition on exactly what the kernels read.  Channel means are offset by up to
    `offset` spreads.  Residuals of kind "p2" hold values their planes represent exactly; res2's planes get a loose scale (2^6 above
    its maximum), so the two residuals' 2^-s differ."""
    rng = np.random.default_rng(seed)
    ho, wo = h << up, w << up
    want = lambda shape: rng.choice([-1.0, 1.0], shape) * (0.25 + np.abs(rng.standard_normal(shape)))
    gamma0 = rng.choice([-1.0, 1.0], c) * rng.uniform(0.5, 1.5, c)
    beta0 = 0.5 * rng.standard_normal(c)
    mu0 = offset * rng.uniform(-1.0, 1.0, c)
    is0 = rng.uniform(0.5, 2.0, c)
    d = dict(n=n, h=h, w=w, c=c, up=up, relu=relu, ho=ho, wo=wo, m=n * h * w, mo=n * ho * wo, kinds=kinds, r=[None, None], rp=[None, None])

    def settle(i, val):
        v = val.astype(np.float32)
        if kinds[i] == "p2":
            s = bo.p2_scale(float(np.abs(v).max()) * (1.5 if i == 0 else 100.0))
            halves = bo.p2_encode(v, s)
            v = bo.p2_decode(halves, 2.0 ** -s, n, c, ho, wo).astype(np.float32)
            d["rp"][i] = (halves, s)
        d["r"][i] = v

    present = [i for i in (0, 1) if kinds[i] != "none"]
    if up == 0:
        pre = want((n, ho, wo, c))
        for i in present:
            settle(i, rng.standard_normal((n, ho, wo, c)) * (1.0 if i == 0 else 8.0))
        y = pre - sum(d["r"][i].astype(np.float64) for i in present)
    elif not present:
        y = want((n, h, w, c))
    else:
        y = rng.standard_normal((n, h, w, c))
        pre = want((n, ho, wo, c))
        for i in present[:-1]:
            settle(i, rng.standard_normal((n, ho, wo, c)))
        settle(present[-1], pre - bo.upsample(y, up) - sum(d["r"][i].astype(np.float64) for i in present[:-1]))
    z = ((y - beta0) / (is0 * gamma0) + mu0).astype(np.float32)
    st = bo.batch_stats(z, BN_EPS)
    mu_t, is_t = st["mean"][0], st["invstd"][0]
    gamma = gamma0 * is0 / is_t
    beta = beta0 - (mu0 - mu_t) * is_t * gamma
    d.update(z=z, mean=mu_t.astype(np.float32), invstd=is_t.astype(np.float32), gamma=gamma.astype(np.float32), beta=beta.astype(np.float32),
             mean64=mu_t, invstd64=is_t)
    return d


def forward_oracle(d, stat_err=False):
    mean, invstd = (d["mean64"], d["invstd64"]) if stat_err else (d["mean"], d["invstd"])
    return bo.bn_forward(d["z"], mean, invstd, d["gamma"], d["beta"], d["up"], d["relu"], d["r"][0], d["r"][1], stat_err=stat_err)


def forward_p2_bound(d):
    rmax = [0.0 if r is None else float(np.abs(r).max()) for r in d["r"]]
    return bo.fwd_bound(d["gamma"], d["beta"], d["m"], rmax[0], rmax[1])


def backward_inputs(d, seed, gscale=1.0):
    """`out` (the float32 of the oracle's forward: an INPUT of the backward), its mask bytes and an output gradient."""
    rng = np.random.default_rng(seed + 17)
    out = forward_oracle(d)["out"].astype(np.float32)
    gout = (gscale * rng.standard_normal(out.shape) * 2.0 ** rng.integers(-3, 4, size=(1, 1, 1, d["c"]))).astype(np.float32)
    return out, bo.mask_bits(out), gout


def fused_case(case):
    """(d, out, bits, gout, relu) of a FUSED_CASES / BWD_P2_CASES / CHAIN_CASES row: the residual kinds follow the mask mode."""
    n, h, w, c, mode = case[:5]
    slots = case[5] if len(case) > 5 else ((0, 0) if mode == 2 else (1, 1))
    kinds = tuple("f32" if s else "none" for s in slots)
    assert (mode == 2) == (mode != 0 and slots == (0, 0)), "mask mode 2 is the ReLU op without residuals, 1 and 3 have some"
    d = make_case(n, h, w, c, 0, int(mode != 0), kinds, _seed(case))
    return (d,) + backward_inputs(d, _seed(case)) + (int(mode != 0),)


def fused_oracle(d, out, bits, gout, mode):
    g = bo.masked_gradient(gout, mode, out=out, bits=bits, z=d["z"], mean=d["mean"], invstd=d["invstd"], gamma=d["gamma"], beta=d["beta"])
    r = bo.bn_backward(g, d["z"], d["mean"], d["invstd"], d["gamma"])
    r["g"] = g
    r["p2_bound"] = bo.bwd_bound(d["gamma"], d["invstd"], float(np.abs(g).max()), r["dbeta"][0], r["dgamma"][0], d["m"])
    return r


# ---- device buffers ---------------------------------------------------------------------------------------------------------------
class Buf:
    """nbytes of output between two guards, one allocation, all of it the NaN pattern unless `init` (a numpy array) is given."""

    def __init__(self, dev, nbytes, init=None):
        self.nbytes = int(nbytes)
        nd = (self.nbytes + 15) // 16 * 4
        self.raw = torch.full((GUARD + nd + GUARD,), SENT, dtype=torch.int32, device=dev)
        if init is not None:
            a = np.ascontiguousarray(init)
            assert a.nbytes == self.nbytes
            self.t(a.dtype.type).copy_(torch.from_numpy(a.reshape(-1)))

    def t(self, np_dtype):
        return self.raw.view(torch.uint8)[GUARD * 4:GUARD * 4 + self.nbytes].view(_TORCH[np_dtype])

    def host(self, np_dtype):
        return self.t(np_dtype).cpu().numpy()

    def guards_ok(self):
        b = self.raw.cpu().numpy().view(np.uint8)
        ref = np.full(self.raw.numel(), SENT, dtype=np.int32).view(np.uint8)
        lo, hi = GUARD * 4, GUARD * 4 + self.nbytes
        return np.array_equal(b[:lo], ref[:lo]) and np.array_equal(b[hi:], ref[hi:])

    def untouched(self):
        return bool((self.raw == SENT).all())

    def written(self):
        """No element still holds the prefill (dword-wise; byte-wise for the mask bytes, which are all below 16)."""
        if self.nbytes % 4:
            return bool((self.host(np.uint8) < 16).all())
        return bool((self.t(np.int32) != SENT).all())


def _zeros(dev, nbytes):
    return Buf(dev, nbytes, np.zeros(nbytes, dtype=np.uint8))


class Lib:
    def __init__(self):
        from multi_view_active_learning_amd import _lib

        self.lib, self.st, self._p, self.check = _lib.lib(), _lib._stream(), _lib._p, _lib._check

    def p(self, x):
        if x is None:
            return C.c_void_p(0)
        return self._p(x.t(np.uint8) if isinstance(x, Buf) else x)

    def last_error(self):
        m = self.lib.mval_last_error()
        return m.decode() if m else ""


ci = C.c_int


def _in(dev, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _bits(v):
    return int(np.float32(v).view(np.int32))


def mag_row(values):
    """[count = 3, partials]: two below the tensor's maximum, the maximum itself in the LAST one."""
    mx = float(np.abs(values).max())
    row = np.zeros(ROW, dtype=np.int32)
    row[0] = 3
    row[1:4] = [_bits(mx / 64.0), _bits(mx / 8.0), _bits(mx)]
    return row


def p2_rows_of(n, s):
    rows = np.zeros((n, bo.P2_ROW), dtype=np.int32)
    rows[:, bo.P2_INV_SLOT] = bo.p2_inv_bits(s)
    return rows


def ratio(got, want, bound):
    err = np.abs(np.asarray(got, dtype=np.float64) - want)
    assert np.isfinite(err).all()
    return float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0.0


def check_amax_row(row, nb, values, what):
    """row[0] = the grid, one partial per workgroup, their maximum bit-equal to max |values| of the downloaded tensor, nothing past them."""
    assert row.guards_ok(), what
    r = row.host(np.int32)
    assert r[0] == nb, (what, int(r[0]), nb)
    assert (r[1:1 + nb] != SENT).all(), what
    assert int(r[1:1 + nb].max()) == _bits(np.abs(values).max()), what
    assert (r[1 + nb:] == SENT).all(), what


def check_p2_rows(rows, n, s, what):
    assert rows.guards_ok(), what
    r = rows.host(np.int32).reshape(n, bo.P2_ROW)
    assert (r[:, bo.P2_INV_SLOT] == bo.p2_inv_bits(s)).all(), (what, [hex(int(v)) for v in r[:, bo.P2_INV_SLOT]], hex(bo.p2_inv_bits(s)))
    assert not r[:, :bo.P2_INV_SLOT].any(), what


def check_planes(planes, x_dev, s, n, c, h, w, what):
    """Planes of the tensor whose fp32 copy the same launch wrote (x_dev): plane 0 is h = fp16(x * 2^s) itself (normal range), and
    (h + l) * 2^-s is within the format's statement of x.  Returns the worst error / bound."""
    assert planes.guards_ok() and planes.written(), what
    halves = planes.host(np.float16)
    inv = 2.0 ** -s
    hi, _ = bo.p2_planes(halves, n, c, h, w)
    v = x_dev.astype(np.float32) * np.float32(2.0 ** s)
    normal = (np.abs(v) >= 2.0 ** -14) | (v == 0)
    assert np.array_equal(hi[normal], v.astype(np.float16).astype(np.float64)[normal]), what + ": plane 0 is not fp16(x * 2^s)"
    return ratio(bo.p2_decode(halves, inv, n, c, h, w), x_dev.astype(np.float64), bo.p2_format_bound(x_dev, inv))


# ---- batch statistics -------------------------------------------------------------------------------------------------------------
def stats_data(case):
    """z whose channel means sit up to 100 spreads from zero (E[z^2] - mean^2 cancels), spreads 2^-2 .. 2^2."""
    n, h, w, c = case
    rng = np.random.default_rng(_seed(case))
    spread = 2.0 ** rng.integers(-2, 3, size=c)
    off = rng.uniform(-100.0, 100.0, size=c) * spread
    off[0] = 100.0 * spread[0]
    return (rng.standard_normal((n, h, w, c)) * spread + off).astype(np.float32)


def _check_stats(want, mean, invstd, rm, rv, tag):
    worst = {}
    for name, buf in (("mean", mean), ("invstd", invstd), ("running_mean", rm), ("running_var", rv)):
        if buf is None:
            continue
        assert buf.guards_ok() and buf.written(), (tag, name)
        worst[name] = ratio(buf.host(np.float32), *want[name])
    print(f"[bn stats] {tag}: ratio " + " ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert max(worst.values()) <= 1.0, (tag, worst)


@gpu
@pytest.mark.parametrize("case", STATS_CASES, ids=_id)
def test_batch_stats_vs_float64(dev, case):
    L = Lib()
    n, h, w, c = case
    m = n * h * w
    z = stats_data(case)
    rng = np.random.default_rng(3)
    rm0, rv0 = rng.standard_normal(c).astype(np.float32), rng.uniform(0.5, 2.0, c).astype(np.float32)
    want = bo.batch_stats(z, BN_EPS, 0.1, rm0, rv0)
    zd = _in(dev, z)
    for running in (1, 0):
        mean, invstd, ws = Buf(dev, 4 * c), Buf(dev, 4 * c), Buf(dev, 512 * c * 2 * 8)
        rm, rv = (Buf(dev, 4 * c, rm0), Buf(dev, 4 * c, rv0)) if running else (None, None)
        L.check(L.lib.mval_bn_batch_stats(L.p(zd), C.c_int64(m), ci(c), C.c_float(BN_EPS), C.c_float(0.1), L.p(mean), L.p(invstd), L.p(rm), L.p(rv),
                                          L.p(ws), L.st), "batch stats")
        assert ws.guards_ok()
        _check_stats(want, mean, invstd, rm, rv, f"{case} running={running}")


@gpu
def test_finalize_stats_tiles_vs_float64(dev):
    """mval_bn_finalize_stats on part[c][tiles][2] float64 partials of 300 tiles (more than its 256 threads: the loop's second trip, ragged)."""
    L = Lib()
    n, h, w, c, tiles = TILES_CASE
    m = n * h * w
    z = stats_data((n, h, w, c))
    zz = z.reshape(m, c).astype(np.float64)
    part = np.zeros((c, tiles, 2))
    for t, idx in enumerate(np.array_split(np.arange(m), tiles)):
        part[:, t, 0], part[:, t, 1] = zz[idx].sum(0), (zz[idx] ** 2).sum(0)
    rng = np.random.default_rng(4)
    rm0, rv0 = rng.standard_normal(c).astype(np.float32), rng.uniform(0.5, 2.0, c).astype(np.float32)
    want = bo.batch_stats(z, BN_EPS, 0.1, rm0, rv0)
    pd = _in(dev, part)
    for running in (1, 0):
        mean, invstd = Buf(dev, 4 * c), Buf(dev, 4 * c)
        rm, rv = (Buf(dev, 4 * c, rm0), Buf(dev, 4 * c, rv0)) if running else (None, None)
        L.check(L.lib.mval_bn_finalize_stats(L.p(pd), ci(tiles), C.c_int64(m), ci(c), C.c_float(BN_EPS), C.c_float(0.1), L.p(mean), L.p(invstd),
                                             L.p(rm), L.p(rv), L.st), "finalize stats")
        _check_stats(want, mean, invstd, rm, rv, f"tiles {TILES_CASE} running={running}")


# ---- forward apply, fp32 ----------------------------------------------------------------------------------------------------------
def _stat_inputs(dev, d):
    return [_in(dev, d[k]) for k in ("z", "mean", "invstd", "gamma", "beta")]


@gpu
@pytest.mark.parametrize("case", FWD_CASES, ids=_id)
def test_apply_fwd_fp32_vs_float64(dev, case):
    """mval_bn_apply_fwd, _amax and _mask: out against the oracle, the mask bytes = the bits of the device's out, the magnitude row."""
    L = Lib()
    n, h, w, c, up, relu, kinds = case
    d = make_case(n, h, w, c, up, relu, kinds, _seed(case))
    o = forward_oracle(d)
    nb = bo.launch_geometry("apply", c, d["m"], d["mo"])["nb"]
    zd, md, isd, gd, bd = _stat_inputs(dev, d)
    rd = [None if r is None else _in(dev, r) for r in d["r"]]
    dims = (ci(n), ci(h), ci(w), ci(c), ci(up), ci(relu))
    first = None
    for entry in ("plain", "amax", "mask"):
        out, row, mask = Buf(dev, 4 * d["mo"] * c), Buf(dev, 4 * ROW), Buf(dev, d["mo"] * c // 4)
        head = (L.p(zd), L.p(md), L.p(isd), L.p(gd), L.p(bd), L.p(rd[0]), L.p(rd[1]), L.p(out)) + dims
        if entry == "plain":
            L.check(L.lib.mval_bn_apply_fwd(*head, L.st), entry)
        elif entry == "amax":
            L.check(L.lib.mval_bn_apply_fwd_amax(*head, L.p(row), L.st), entry)
        else:
            L.check(L.lib.mval_bn_apply_fwd_mask(*head, L.p(row), L.p(mask), L.st), entry)
        assert out.guards_ok() and out.written(), entry
        got = out.host(np.float32).reshape(o["out"].shape)
        if first is None:
            first = got
            e = ratio(got, o["out"], o["bound"])
            print(f"[bn apply fwd] {_id(case)}: ratio {e:.3f}")
            assert e <= 1.0, e
        assert np.array_equal(got.view(np.int32), first.view(np.int32)), entry
        if entry == "plain":
            assert row.untouched()
        else:
            check_amax_row(row, nb, got, entry)
        if entry == "mask":
            assert mask.guards_ok() and mask.written()
            assert np.array_equal(mask.host(np.uint8), bo.mask_bits(got))
        else:
            assert mask.untouched()


# ---- forward apply, P2 ------------------------------------------------------------------------------------------------------------
def run_fwd_p2(L, dev, d, stats=None, with_out=True, what="fwd p2"):
    """One launch of mval_bn_apply_fwd_p2 (no residual kept as planes) or mval_bn_apply_fwd_p2_res; returns the guarded outputs."""
    n, h, w, c, up, relu = (d[k] for k in ("n", "h", "w", "c", "up", "relu"))
    zd, md, isd, gd, bd = _stat_inputs(dev, d)
    if stats is not None:
        md, isd = stats
    mo = d["mo"]
    r = dict(out=Buf(dev, 4 * mo * c) if with_out else None, planes=Buf(dev, 4 * mo * c), rows=_zeros(dev, 4 * n * bo.P2_ROW), row=Buf(dev, 4 * ROW),
             mask=Buf(dev, mo * c // 4))
    f32 = [(_in(dev, d["r"][i]) if d["kinds"][i] == "f32" else None) for i in (0, 1)]
    mrow = [(_in(dev, mag_row(d["r"][i])) if d["kinds"][i] != "none" else None) for i in (0, 1)]
    pl = [(_in(dev, d["rp"][i][0]) if d["kinds"][i] == "p2" else None) for i in (0, 1)]
    prow = [(_in(dev, p2_rows_of(n, d["rp"][i][1])) if d["kinds"][i] == "p2" else None) for i in (0, 1)]
    head = (L.p(zd), L.p(md), L.p(isd), L.p(gd), L.p(bd), L.p(f32[0]), L.p(f32[1]), L.p(r["out"]), L.p(r["planes"]), L.p(r["rows"]), ci(n), ci(h), ci(w),
            ci(c), ci(up), ci(relu), L.p(r["row"]), L.p(r["mask"]), L.p(mrow[0]), L.p(mrow[1]))
    if "p2" in d["kinds"]:
        L.check(L.lib.mval_bn_apply_fwd_p2_res(*head, L.p(pl[0]), L.p(prow[0]), L.p(pl[1]), L.p(prow[1]), L.st), what)
    else:
        L.check(L.lib.mval_bn_apply_fwd_p2(*head, L.st), what)
    torch.cuda.synchronize()
    return r


def check_fwd_p2(d, r, o, bound, tag):
    n, c, ho, wo = d["n"], d["c"], d["ho"], d["wo"]
    nb = bo.launch_geometry("apply_p2", c, d["m"], d["mo"])["nb"]
    s = bo.p2_scale(bound)
    assert r["out"].guards_ok() and r["out"].written()
    got = r["out"].host(np.float32).reshape(n, ho, wo, c)
    e = ratio(got, o["out"], o["bound"])
    check_amax_row(r["row"], nb, got, tag)
    assert r["mask"].guards_ok() and r["mask"].written()
    assert np.array_equal(r["mask"].host(np.uint8), bo.mask_bits(got)), tag
    check_p2_rows(r["rows"], n, s, tag)
    ep = check_planes(r["planes"], got, s, n, c, ho, wo, tag)
    print(f"[bn apply fwd p2] {tag}: ratio out {e:.3f} planes {ep:.3f}")
    assert e <= 1.0 and ep <= 1.0, (e, ep)
    return got


@gpu
@pytest.mark.parametrize("case", FWD_P2_CASES, ids=_id)
def test_apply_fwd_p2_vs_float64(dev, case):
    L = Lib()
    n, h, w, c, up, relu, kinds = case
    d = make_case(n, h, w, c, up, relu, kinds, _seed(case))
    r = run_fwd_p2(L, dev, d)
    check_fwd_p2(d, r, forward_oracle(d), forward_p2_bound(d), _id(case))
    r0 = run_fwd_p2(L, dev, d, with_out=False)  # out = NULL: the same planes, rows, mask and magnitude row
    for k in ("planes", "rows", "row", "mask"):
        assert r0[k].guards_ok() and torch.equal(r0[k].raw, r[k].raw), k


@gpu
@pytest.mark.parametrize("case", PLANE_STATS_CASES, ids=_id)
def test_p2_plane_stats_exact(dev, case):
    """All four dwords of mval_p2_plane_stats equal what the host computes from the downloaded planes (float32 h + l, as the kernel)."""
    L = Lib()
    n, h, w, c, up, relu, kinds = case
    d = make_case(n, h, w, c, up, relu, kinds, _seed(case))
    r = run_fwd_p2(L, dev, d)
    out4 = _zeros(dev, 16)
    L.check(L.lib.mval_p2_plane_stats(L.p(r["planes"]), L.p(r["rows"]), ci(n), ci(c), ci(d["ho"] * d["wo"]), L.p(out4), L.st), "plane stats")
    assert out4.guards_ok()
    a = r["planes"].host(np.float16).reshape(n, 2, -1).astype(np.float32)
    v = np.abs(a[:, 0] + a[:, 1])
    want = [int(r["rows"].host(np.int32)[bo.P2_INV_SLOT]), _bits(v.max()), int(((v > 0) & (v < 0.125)).sum()), int((v > 0).sum())]
    got = [int(x) for x in out4.host(np.int32).view(np.uint32)]
    print(f"[p2 plane stats] {_id(case)}: {got}")
    assert got == [x & 0xFFFFFFFF for x in want], (got, want)


@gpu
def test_p2_plane_stats_counts_small_values(dev):
    """The forward's planes hold nothing below 2^-3 scaled (|pre-activation| >= 0.25 by construction), so the `small` count above is 0:
    here host-encoded planes of values spread over 2^-30 .. 2^4 with exact zeros, counted exactly."""
    L = Lib()
    n, h, w, c = 3, 5, 3, 24
    rng = np.random.default_rng(5)
    x = (rng.standard_normal((n, h, w, c)) * 2.0 ** rng.integers(-30, 5, size=(n, h, w, c))).astype(np.float32)
    x[rng.random(x.shape) < 0.1] = 0.0
    s = bo.p2_scale(float(np.abs(x).max()) * 3.0)
    halves = bo.p2_encode(x, s)
    a = halves.reshape(n, 2, -1).astype(np.float32)
    v = np.abs(a[:, 0] + a[:, 1])
    want = [bo.p2_inv_bits(s), _bits(v.max()), int(((v > 0) & (v < 0.125)).sum()), int((v > 0).sum())]
    assert 0 < want[2] < want[3] < x.size
    out4, planes, rows = _zeros(dev, 16), _in(dev, halves), _in(dev, p2_rows_of(n, s))
    L.check(L.lib.mval_p2_plane_stats(L.p(planes), L.p(rows), ci(n), ci(c), ci(h * w), L.p(out4), L.st), "plane stats")
    assert out4.guards_ok()
    got = [int(t) for t in out4.host(np.int32).view(np.uint32)]
    print(f"[p2 plane stats] small values: {got}")
    assert got == want, (got, want)


# ---- backward, fp32 ---------------------------------------------------------------------------------------------------------------
def _gres_bufs(dev, slots, overwrite, shape, seed):
    """The two residual-gradient slots: a stored one keeps the NaN prefill (stale), an accumulated one starts from known contents."""
    rng = np.random.default_rng(seed + 29)
    bufs, prior = [None, None], [None, None]
    for i in (0, 1):
        if slots[i]:
            if not (overwrite >> i) & 1:
                prior[i] = rng.standard_normal(shape).astype(np.float32)
            bufs[i] = Buf(dev, 4 * int(np.prod(shape)), prior[i])
    return bufs, prior


def _check_gres(bufs, prior, slots, overwrite, g, tag):
    worst = 0.0
    for i in (0, 1):
        if slots[i]:
            assert bufs[i].guards_ok() and bufs[i].written(), (tag, i)
            want, bound = bo.residual_gradient(g, prior[i], (overwrite >> i) & 1)
            worst = max(worst, ratio(bufs[i].host(np.float32).reshape(g.shape), want, bound))
    return worst


def _check_vec(buf, want, tag):
    assert buf.guards_ok() and buf.written(), tag
    return ratio(buf.host(np.float32), *want)


@gpu
@pytest.mark.parametrize("case", BWD_CASES, ids=_id)
def test_bn_bwd_vs_float64(dev, case):
    """mval_bn_bwd and mval_bn_bwd_amax: the window sum over the replicas, both residual slots stored or accumulated per `overwrite` bit,
    has_bn 0 and 1."""
    L = Lib()
    n, h, w, c, up, relu, has_bn, slots, overwrite = case
    d = make_case(n, h, w, c, up, relu, tuple("f32" if s else "none" for s in slots), _seed(case))
    out, _, gout = backward_inputs(d, _seed(case))
    g = bo.masked_gradient(gout, 1 if relu else 0, out=out)
    want = bo.bn_backward(g, d["z"], d["mean"], d["invstd"], d["gamma"], up, has_bn)
    nb2 = bo.launch_geometry("apply", c, d["m"])["nb"]
    zd, md, isd, gd, _ = _stat_inputs(dev, d)
    goutd, outd = _in(dev, gout), _in(dev, out)
    first = None
    for entry in ("plain", "amax"):
        gres, prior = _gres_bufs(dev, slots, overwrite, g.shape, _seed(case))
        gz, dg, db, ws, sums, row = Buf(dev, 4 * d["m"] * c), Buf(dev, 4 * c), Buf(dev, 4 * c), Buf(dev, 512 * c * 2 * 8), Buf(dev, 8 * c), Buf(dev, 4 * ROW)
        head = (L.p(goutd), L.p(outd), L.p(zd), L.p(md), L.p(isd), L.p(gd), L.p(gres[0]), L.p(gres[1]), L.p(gz), L.p(dg), L.p(db), L.p(ws), L.p(sums), ci(n),
                ci(h), ci(w), ci(c), ci(up), ci(relu), ci(has_bn), ci(overwrite))
        if entry == "plain":
            L.check(L.lib.mval_bn_bwd(*head, L.st), entry)
        else:
            L.check(L.lib.mval_bn_bwd_amax(*head, L.p(row), L.st), entry)
        assert gz.guards_ok() and gz.written() and ws.guards_ok() and sums.guards_ok() and sums.written(), entry
        got = gz.host(np.float32).reshape(n, h, w, c)
        e = dict(gres=_check_gres(gres, prior, slots, overwrite, g, entry), dbeta=_check_vec(db, want["dbeta"], entry))
        if has_bn:
            e["dgamma"] = _check_vec(dg, want["dgamma"], entry)
            e["dz"] = ratio(got, *want["dz"])
            assert np.array_equal(sums.host(np.float32), np.concatenate([db.host(np.float32), dg.host(np.float32)]))
        else:
            e["gz"] = ratio(got, *want["gz"])
            assert dg.untouched()
        if entry == "amax" and has_bn:
            check_amax_row(row, nb2, got, entry)
        else:
            assert row.untouched()
        if first is None:
            first = got
            print(f"[bn bwd] {_id(case)}: ratio " + " ".join(f"{k} {v:.3f}" for k, v in e.items()))
        assert max(e.values()) <= 1.0, (entry, e)
        assert np.array_equal(got.view(np.int32), first.view(np.int32)), entry


@gpu
@pytest.mark.parametrize("case", SCALAR_CASES, ids=_id)
def test_bn_bwd_scalar_form_vs_float64(dev, case):
    """mval_bn_bwd at a channel count that is no multiple of 4 (bias_bwd_scalar_kernel): gz = the masked gradient exactly, dbeta its sum."""
    L = Lib()
    n, h, w, c, relu = case
    rng = np.random.default_rng(_seed(case))
    shape = (n, h, w, c)
    out = (rng.choice([-1.0, 1.0], shape) * (0.25 + np.abs(rng.standard_normal(shape)))).astype(np.float32)
    out = np.maximum(out, 0) if relu else out
    gout = rng.standard_normal(shape).astype(np.float32)
    g = bo.masked_gradient(gout, 1 if relu else 0, out=out)
    want = bo.bn_backward(g, None, None, None, None, 0, False)
    gz, db, ws, sums = Buf(dev, 4 * g.size), Buf(dev, 4 * c), Buf(dev, 512 * c * 2 * 8), Buf(dev, 8 * c)
    goutd, outd = _in(dev, gout), _in(dev, out)
    L.check(L.lib.mval_bn_bwd(L.p(goutd), L.p(outd), L.p(None), L.p(None), L.p(None), L.p(None), L.p(None), L.p(None), L.p(gz), L.p(None), L.p(db),
                              L.p(ws), L.p(sums), ci(n), ci(h), ci(w), ci(c), ci(0), ci(relu), ci(0), ci(0), L.st), "bwd scalar")
    assert gz.guards_ok() and gz.written() and ws.guards_ok() and sums.untouched()
    assert np.array_equal(gz.host(np.float32).reshape(shape), g.astype(np.float32))
    e = _check_vec(db, want["dbeta"], "scalar")
    print(f"[bn bwd scalar] {_id(case)}: ratio dbeta {e:.3f}")
    assert e <= 1.0, e


def run_fused(L, dev, d, out, bits, gout, mode, slots, overwrite, p2, with_gz=True, seed=0, stats=None, mask_dev=None, out_dev=None):
    """One launch of mval_bn_bwd_fused (modes 0, 1, 2), mval_bn_bwd_fused_mask (mode 3: `out` is NULL, only the bytes are given) or, with p2,
    mval_bn_bwd_fused_p2 with dz_planes."""
    n, h, w, c, m = (d[k] for k in ("n", "h", "w", "c", "m"))
    zd, md, isd, gd, bd = _stat_inputs(dev, d)
    if stats is not None:
        md, isd = stats
    goutd = _in(dev, gout)
    outd = (out_dev if out_dev is not None else _in(dev, out)) if mode == 1 else None
    maskd = (mask_dev if mask_dev is not None else _in(dev, bits)) if mode == 3 else None
    gres, prior = _gres_bufs(dev, slots, overwrite, gout.shape, seed)
    r = dict(gres=gres, prior=prior, gz=Buf(dev, 4 * m * c) if with_gz else None, dg=Buf(dev, 4 * c), db=Buf(dev, 4 * c), ws=Buf(dev, 512 * c * 2 * 8),
             sums=Buf(dev, 8 * c), row=Buf(dev, 4 * ROW))
    tail = (L.p(zd), L.p(md), L.p(isd), L.p(gd), L.p(bd), L.p(gres[0]), L.p(gres[1]), L.p(r["gz"]), L.p(r["dg"]), L.p(r["db"]), L.p(r["ws"]), L.p(r["sums"]),
            ci(n), ci(h), ci(w), ci(c), ci(int(mode != 0)), ci(overwrite), L.p(r["row"]))
    if p2:
        r.update(planes=Buf(dev, 4 * m * c), rows=_zeros(dev, 4 * n * bo.P2_ROW), gmax=Buf(dev, 4 * 512),
                 slot=Buf(dev, 4, np.array([1e30], dtype=np.float32)))  # (a stale large bound: the call must reset it)
        L.check(L.lib.mval_bn_bwd_fused_p2(L.p(goutd), L.p(outd), L.p(maskd), *tail, L.p(r["planes"]), L.p(r["rows"]), L.p(r["gmax"]), L.p(r["slot"]), L.st),
                "bwd fused p2")
    elif mode == 3:
        L.check(L.lib.mval_bn_bwd_fused_mask(L.p(goutd), L.p(None), L.p(maskd), *tail, L.st), "bwd fused mask")
    else:
        L.check(L.lib.mval_bn_bwd_fused(L.p(goutd), L.p(outd), *tail, L.st), "bwd fused")
    torch.cuda.synchronize()
    return r


def check_fused(d, r, want, slots, overwrite, tag, with_gz=True):
    n, h, w, c = d["n"], d["h"], d["w"], d["c"]
    assert r["ws"].guards_ok() and r["sums"].guards_ok() and r["sums"].written()
    e = dict(gres=_check_gres(r["gres"], r["prior"], slots, overwrite, want["g"], tag), dbeta=_check_vec(r["db"], want["dbeta"], tag),
             dgamma=_check_vec(r["dg"], want["dgamma"], tag))
    assert np.array_equal(r["sums"].host(np.float32), np.concatenate([r["db"].host(np.float32), r["dg"].host(np.float32)]))
    got = None
    if with_gz:
        assert r["gz"].guards_ok() and r["gz"].written()
        got = r["gz"].host(np.float32).reshape(n, h, w, c)
        e["dz"] = ratio(got, *want["dz"])
        check_amax_row(r["row"], bo.launch_geometry("apply", c, d["m"])["nb"], got, tag)
    return e, got


@gpu
@pytest.mark.parametrize("case", FUSED_CASES, ids=_id)
def test_bn_bwd_fused_vs_float64(dev, case):
    L = Lib()
    n, h, w, c, mode, slots, overwrite = case
    d, out, bits, gout, relu = fused_case(case)
    want = fused_oracle(d, out, bits, gout, mode)
    r = run_fused(L, dev, d, out, bits, gout, mode, slots, overwrite, p2=False, seed=_seed(case))
    e, _ = check_fused(d, r, want, slots, overwrite, _id(case))
    print(f"[bn bwd fused] {_id(case)}: ratio " + " ".join(f"{k} {v:.3f}" for k, v in e.items()))
    assert max(e.values()) <= 1.0, e


# ---- backward, P2 -----------------------------------------------------------------------------------------------------------------
BOUND_SLOT_ROUNDINGS = 14  # of bd in bn_bwd_finalize_bound_kernel: two casts, inv_m, sqrt_m1, 1 + 1e-5f, five products, two sums, + 1


def check_bwd_p2(d, r, want, got_gz, tag):
    """dz_rows, the bound left in bound_slot, and the planes: against the fp32 dz of the same launch when it wrote one (plane 0 = h, the
    format's statement), else against the oracle's dz (the format's statement plus the dz tolerance)."""
    n, h, w, c = d["n"], d["h"], d["w"], d["c"]
    s = bo.p2_scale(want["p2_bound"])
    check_p2_rows(r["rows"], n, s, tag)
    assert r["slot"].guards_ok() and r["gmax"].guards_ok()
    left = float(r["slot"].host(np.float32)[0])
    assert abs(left / want["p2_bound"] - 1.0) <= BOUND_SLOT_ROUNDINGS * bo.EPS, (tag, left, want["p2_bound"])
    assert r["planes"].guards_ok() and r["planes"].written()
    dz, e_dz = want["dz"]
    inv = 2.0 ** -s
    dec = bo.p2_decode(r["planes"].host(np.float16), inv, n, c, h, w)
    e = ratio(dec, dz, bo.p2_format_bound(np.abs(dz) + e_dz, inv) + e_dz)
    if got_gz is not None:
        e = max(e, check_planes(r["planes"], got_gz, s, n, c, h, w, tag))
    return e


@gpu
@pytest.mark.parametrize("case", BWD_P2_CASES, ids=_id)
def test_bn_bwd_fused_p2_vs_float64(dev, case):
    L = Lib()
    n, h, w, c, mode, slots, overwrite = case
    d, out, bits, gout, relu = fused_case(case)
    want = fused_oracle(d, out, bits, gout, mode)
    r = run_fused(L, dev, d, out, bits, gout, mode, slots, overwrite, p2=True, seed=_seed(case))
    e, got = check_fused(d, r, want, slots, overwrite, _id(case))
    e["planes"] = check_bwd_p2(d, r, want, got, _id(case))
    print(f"[bn bwd fused p2] {_id(case)}: ratio " + " ".join(f"{k} {v:.3f}" for k, v in e.items()))
    assert max(e.values()) <= 1.0, e
    r0 = run_fused(L, dev, d, out, bits, gout, mode, slots, overwrite, p2=True, with_gz=False, seed=_seed(case))  # gz = NULL: identical planes
    e0, _ = check_fused(d, r0, want, slots, overwrite, _id(case), with_gz=False)
    assert max(e0.values()) <= 1.0, e0
    for k in ("planes", "rows", "row", "slot"):
        assert r0[k].guards_ok() and torch.equal(r0[k].raw, r[k].raw), k


# ---- one chain per mask mode ------------------------------------------------------------------------------------------------------
def chain_reference(d, gout):
    """float64 torch.autograd of the whole operator on the float32 inputs: (out, dz, dgamma, dbeta, residual gradients), NHWC."""
    import torch.nn.functional as F

    t = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float64))).requires_grad_(True)
    z, gamma, beta = t(d["z"]), t(d["gamma"]), t(d["beta"])
    res = [t(r) for r in d["r"] if r is not None]
    y = F.batch_norm(z.permute(0, 3, 1, 2), None, None, gamma, beta, True, 0.1, float(np.float32(BN_EPS))).permute(0, 2, 3, 1)
    for r in res:
        y = y + r
    if d["relu"]:
        y = F.relu(y)
    y.backward(torch.from_numpy(gout.astype(np.float64)))
    return y.detach().numpy(), z.grad.numpy(), gamma.grad.numpy(), beta.grad.numpy(), [r.grad.numpy() for r in res]


@gpu
@pytest.mark.parametrize("case", CHAIN_CASES, ids=_id)
def test_chain_stats_fwd_p2_bwd_p2_vs_autograd(dev, case):
    """mval_bn_batch_stats -> mval_bn_apply_fwd_p2 -> mval_bn_bwd_fused_p2, each reading what the one before left on the device, against
    float64 autograd.  The device only has mean and invstd rounded to float32: the oracle's bounds with stat_err."""
    L = Lib()
    n, h, w, c, mode = case
    d, _, _, gout, relu = fused_case(case)
    slots, m = ((0, 0) if mode == 2 else (1, 1)), d["m"]
    ref_out, ref_dz, ref_dg, ref_db, ref_gres = chain_reference(d, gout)
    o = forward_oracle(d, stat_err=True)
    assert np.abs(o["out"] - ref_out).max() <= 1e-12 * np.abs(ref_out).max()
    mean, invstd, ws, zd = Buf(dev, 4 * c), Buf(dev, 4 * c), Buf(dev, 512 * c * 2 * 8), _in(dev, d["z"])
    L.check(L.lib.mval_bn_batch_stats(L.p(zd), C.c_int64(m), ci(c), C.c_float(BN_EPS), C.c_float(0.1), L.p(mean), L.p(invstd), L.p(None),
                                      L.p(None), L.p(ws), L.st), "chain stats")
    stats = (mean.t(np.float32), invstd.t(np.float32))
    f = run_fwd_p2(L, dev, d, stats=stats)
    got_out = check_fwd_p2(d, f, o, forward_p2_bound(d), "chain " + _id(case))
    g = bo.masked_gradient(gout, 1 if relu else 0, out=ref_out)
    want = bo.bn_backward(g, d["z"], d["mean64"], d["invstd64"], d["gamma"], stat_err=True)
    assert np.abs(want["dz"][0] - ref_dz).max() <= 1e-12 * np.abs(ref_dz).max()
    want.update(g=g, dz=(ref_dz, want["dz"][1]), dgamma=(ref_dg, want["dgamma"][1]), dbeta=(ref_db, want["dbeta"][1]),
                p2_bound=bo.bwd_bound(d["gamma"], d["invstd64"], float(np.abs(g).max()), ref_db, ref_dg, m))
    for gr in ref_gres:  # (autograd's residual gradients are the masked gradient itself)
        assert np.array_equal(gr, g)
    ow = CHAIN_OVERWRITE[mode]
    r = run_fused(L, dev, d, got_out, None, gout, mode, slots, ow, p2=True, seed=_seed(case), stats=stats, mask_dev=f["mask"].t(np.uint8),
                  out_dev=f["out"].t(np.float32))
    e, got = check_fused(d, r, want, slots, ow, "chain", with_gz=True)  # (the slots: stored = g exactly, accumulated = known contents + g)
    e["planes"] = check_bwd_p2(d, r, want, got, "chain")
    print(f"[bn chain] {_id(case)}: ratio " + " ".join(f"{k} {v:.3f}" for k, v in e.items()))
    assert max(e.values()) <= 1.0, e


# ---- argument checks that return before any launch --------------------------------------------------------------------------------
@gpu
def test_argument_checks_return_before_launch(dev):
    L = Lib()
    n, h, w = 2, 3, 3
    f = lambda c: torch.zeros(n * h * w * c, device=dev)
    v = lambda c: torch.ones(c, device=dev)
    row, rows = torch.zeros(ROW, dtype=torch.int32, device=dev), torch.zeros(n * bo.P2_ROW, dtype=torch.int32, device=dev)
    ws, sums, mask = torch.zeros(512 * 32 * 2, dtype=torch.float64, device=dev), torch.zeros(64, device=dev), torch.zeros(n * h * w * 8, dtype=torch.uint8, device=dev)
    gmax, slot = torch.zeros(512, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    p, N = L._p, L._p(None)

    def fwd_p2(c, res1=None, res1_row=None, res1_p2=None, res1_p2_rows=None):
        return L.lib.mval_bn_apply_fwd_p2_res(p(f(c)), p(v(c)), p(v(c)), p(v(c)), p(v(c)), p(res1), N, p(f(c)), p(f(c)), p(rows), ci(n), ci(h), ci(w), ci(c),
                                              ci(0), ci(1), p(row), p(mask), p(res1_row), N, p(res1_p2), p(res1_p2_rows), N, N, L.st)

    def bwd(c, has_bn, g1, g2):
        return L.lib.mval_bn_bwd(p(f(c)), p(f(c)), p(f(c)), p(v(c)), p(v(c)), p(v(c)), p(g1), p(g2), p(f(c)), p(v(c)), p(v(c)), p(ws), p(sums), ci(n), ci(h),
                                 ci(w), ci(c), ci(0), ci(1), ci(has_bn), ci(0), L.st)

    def fused(c, out, maskb, g1, g2, planes=None):
        return L.lib.mval_bn_bwd_fused_p2(p(f(c)), p(out), p(maskb), p(f(c)), p(v(c)), p(v(c)), p(v(c)), p(v(c)), p(g1), p(g2), p(f(c)), p(v(c)), p(v(c)), p(ws),
                                          p(sums), ci(n), ci(h), ci(w), ci(c), ci(1), ci(0), N, p(planes), p(rows) if planes is not None else N,
                                          p(gmax) if planes is not None else N, p(slot) if planes is not None else N, L.st)

    g16 = f(16)
    checks = [
        ("P2 forward with C % 8 != 0", "mval_bn_apply_fwd_p2: bad arguments (C % 8)", lambda: fwd_p2(12)),
        ("a residual without its row", "needs its magnitude row", lambda: fwd_p2(16, res1=f(16))),
        ("a residual as planes without its row", "needs its magnitude row", lambda: fwd_p2(16, res1_p2=f(16), res1_p2_rows=rows)),
        ("a residual as both fp32 and planes", "either as fp32", lambda: fwd_p2(16, res1=f(16), res1_row=row, res1_p2=f(16), res1_p2_rows=rows)),
        ("gres1 == gres2 (mval_bn_bwd)", "mval_bn_bwd: the two residual gradients must be distinct buffers", lambda: bwd(16, 1, g16, g16)),
        ("gres1 == gres2 (fused)", "mval_bn_bwd_fused: the two residual gradients must be distinct buffers", lambda: fused(16, f(16), None, g16, g16)),
        ("ReLU + residual gradients without out or mask", "needs the output activation", lambda: fused(16, None, None, f(16), f(16))),
        ("P2 backward with C % 8 != 0", "C % 8 == 0", lambda: fused(12, None, None, None, None, planes=f(12))),
        ("an odd channel count with has_bn", "odd channel count only for plain conv+bias", lambda: bwd(19, 1, None, None)),
    ]
    for what, fragment, call in checks:
        rc = call()
        assert rc == -1, (what, rc)  # (-1: a refused argument; a launch that failed returns -2)
        assert fragment in L.last_error(), (what, L.last_error())
    torch.cuda.synchronize()
