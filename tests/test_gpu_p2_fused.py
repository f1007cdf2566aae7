"""The four fused P2 launches of a default HRNet forward alone -- the BasicBlock (csrc/conv_block_p2.hip), the Bottleneck (conv_bneck_p2.hip), the
stem (conv_stem_p2.hip) and the fuse-up terms (conv_fuse_up_p2.hip) -- at each of their eleven kernel instances: ragged last tiles, a
workgroup's later tiles, per-image magnitudes that differ, the folded partial maxima (more tiles per image than slots), and what a launch must
not write.

Which tiling a launch runs on is read from the launchers' own dry runs (mval_fused_p2_form: host arithmetic, no GPU; tests/p2_fused.py holds the
tables, the inputs and the float64 references).  The host tests hold every row to the instance and the edge it is in the table for; the GPU
tests run each row against float64 and against the chain of single-conv launches it replaces.

Images differ in magnitude (scaled DOWN only: 2^-10, 2^-4, 1), the Bottleneck's separate residual and the fuse-up terms by factors rotated over
the images: a scale read from another image's row -- image 0's, or the one of the tile the workgroup walked before -- loses ten bits or
overflows fp16."""
import time

import numpy as np
import pytest
import torch

import p2_forms as pf
import p2_fused as fu
from test_gpu_p2 import _report
from test_gpu_p2_forms import NAN_BITS, RMS_MIN_ELEMENTS, _bits_equal, _launch_poisoned
from test_p2_walk_host import walk

gpu = pytest.mark.gpu
RTOL = 1e-4
ATOL = dict(block=2e-5, bneck=3e-5, stem=3e-5, fuse=3e-5)  # the bounds of the four older tests of tests/test_gpu_p2.py
BIG_BITS = 0x49800000  # 2^20 as float32: above every output of the tables
_RATIOS = {}


# ---- host tests (no GPU) ----
@pytest.fixture(scope="module")
def lib():
    from multi_view_active_learning_amd import _lib

    return _lib.lib()


def test_the_query_answers_like_the_support_predicate_and_needs_no_gpu(lib):
    """mval_fused_p2_form answers exactly where mval_op_algo_supported(MVAL_ALGO_MFMA_P2) does, for the four fused kinds only; what it fills."""
    import ctypes as C

    from multi_view_active_learning_amd import _lib
    from multi_view_active_learning_amd.engine import _query_op

    R = fu.Row
    sweep = [R("block_c32", 1, 8, 16), R("block_c32", 2, 7, 16), R("block_c32", 2, 8, 15), R("block_c64", 3, 21, 37), R("block_c48", 2, 16, 16),
             R("block_c128", 2, 16, 16), R("block_c32", 1 << 14, 256, 256),
             R("bneck_c64", 2, 8, 16), R("bneck_c256", 3, 9, 17), R("bneck_c128", 2, 16, 16), R("bneck_c256", 2, 7, 16), R("bneck_c64", 2, 8, 12),
             R("stem", 1, 16, 64), R("stem", 2, 20, 68), R("stem", 2, 18, 64), R("stem", 2, 16, 60), R("stem", 2, 12, 64), R("stem", 3, 256, 256),
             R("fuse_c32", 2, 8, 32, terms=(1, 2)), R("fuse_c32", 2, 12, 40, terms=(1, 2)), R("fuse_c32", 2, 12, 40, terms=(1, 2, 3)),
             R("fuse_c32", 2, 16, 40, terms=(1, 2, 3)), R("fuse_c32", 2, 12, 40, terms=(1,)), R("fuse_c40", 2, 12, 40, terms=(1, 2)),
             R("fuse_c48", 2, 12, 24, terms=(1, 2)), R("fuse_c96", 2, 12, 36, terms=(1, 2)), R("fuse_c96", 2, 16, 40, terms=(1, 2, 3)),
             R("fuse_c96", 2, 10, 40, terms=(1, 2)), R("fuse_c64", 2, 6, 40, terms=(1, 2)), R("fuse_c32", 2, 12, 42, terms=(1, 2))]
    seen = {k: set() for k in ("block", "bneck", "stem", "fuse")}
    for r in sweep:
        op = fu.query_op(r)
        ok = bool(lib.mval_op_algo_supported(C.byref(op), C.c_int(r.n), C.c_int(fu.ALGO_P2)))
        f = fu.form(r)
        assert (f is not None) == ok, fu.row_id(r)
        seen[fu.kind_of(r)].add(ok)
        if ok:
            _, _, ho, wo = fu.out_shape(r)
            d = f.as_dict()
            assert (f.tiles_x, f.tiles_y, f.tiles_total) == (-(-wo // f.tile_w), -(-ho // f.th), -(-wo // f.tile_w) * -(-ho // f.th) * r.n), fu.row_id(r)
            assert (f.groups, f.parities, f.threads) == (1, 1, 256) and 0 < f.smem_bytes <= 160 * 1024
            assert all(v == 0 for k, v in d.items() if k not in ("th", "tile_w", "tiles_x", "tiles_y", "tiles_total", "groups", "parities", "smem_bytes", "threads"))
    assert all(v == {True, False} for v in seen.values()), seen
    # (other kinds, other algos' ops and a batch of none have no fused form)
    conv = _query_op(0, 3, 1, 1, 32, 32, 16, 16, 16, 16, algo=fu.ALGO_P2, res1_off=-1, res2_off=-1, in_amax_off=1, out_amax_off=1)
    assert _lib.fused_p2_form(conv, 2) is None and _lib.fused_p2_form(fu.query_op(R("block_c32", 2, 8, 16)), 0) is None
    f = fu.form(R("block_c32", 2, 21, 37))
    assert (f.th, f.tile_w, f.tiles_x, f.tiles_y, f.tiles_total) == (8, 16, 3, 3, 18)
    f = fu.form(R("stem", 3, 100, 76))
    assert (f.th, f.tile_w, f.tiles_x, f.tiles_y, f.tiles_total) == (2, 16, 2, 13, 78)
    # (fuse-up: the LDS holds every term's low-resolution tile of fp32 results)
    f = fu.form(R("fuse_c48_tw24", 1, 96, 72, terms=(1, 2, 3)))
    assert (f.th, f.tile_w, f.smem_bytes) == (8, 24, (4 * 12 + 2 * 6 + 1 * 3) * 48 * 4)
    f = fu.form(R("fuse_c96_tw36", 2, 48, 36, terms=(1, 2)))
    assert (f.th, f.tile_w, f.tiles_x, f.tiles_y, f.smem_bytes) == (4, 36, 1, 12, (2 * 18 + 1 * 9) * 96 * 4)


def test_every_row_takes_the_instance_it_is_in_the_table_for():
    rows = fu.EDGE_ROWS + fu.LATE_ROWS + fu.FOLD_ROWS
    bad = [(fu.row_id(r), f and fu.instance(r, f)) for r in rows for f in [fu.form(r)] if f is None or fu.instance(r, f) != r.inst]
    assert not bad, bad
    ids = [fu.row_id(r) for r in rows]
    assert len(set(ids)) == len(ids)
    assert all(r.res for r in rows if r.inst == "bneck_c64"), "the Bottleneck from 64 channels has no residual but a separate one"
    for r in rows:  # (the same instance on every batch a test runs the row at)
        assert fu.instance(r, fu.form(r, 1)) == r.inst and (fu.form(r, 1).th, fu.form(r, 1).tile_w) == (fu.form(r).th, fu.form(r).tile_w)


def test_the_tables_name_all_eleven_instances():
    assert len(fu.INSTANCES) == 11 and {r.inst for r in fu.EDGE_ROWS} == set(fu.INSTANCES)
    assert {r.inst for r in fu.LATE_ROWS} == {"block_c32", "block_c64", "bneck_c256", "bneck_c64", "stem"}  # (the persistent kernels)
    assert {r.inst for r in fu.FOLD_ROWS} == {"block_c32", "stem", "fuse_c32", "bneck_c64"}  # (p2_slot_put's fold: one row per launcher)
    assert any(not r.relu for r in fu.EDGE_ROWS if r.inst.startswith("fuse")) and {len(r.terms) for r in fu.EDGE_ROWS if r.terms} == {2, 3}


def test_edge_rows_are_ragged_where_they_claim_to_be():
    """Per instance: a row of one tile per image or of whole tiles only, and (where the support predicate allows it) a row with a partly filled
    last tile in rows and one in columns; three images of three magnitudes each."""
    rag = {}
    for r in fu.EDGE_ROWS:
        assert r.n == 3 and fu.factors(r) == fu.EDGE_FACTORS
        rag.setdefault(r.inst, []).append(fu.ragged(r, fu.form(r)))
    for inst in ("block_c32", "block_c64"):
        assert rag[inst] == [(False, False), (True, True), (True, True)], inst
    assert rag["bneck_c256"] == [(False, False), (True, True), (True, True)] and rag["bneck_c64"] == [(False, False), (True, True)]
    assert rag["stem"] == [(False, False), (True, True), (True, True)]
    assert rag["fuse_c32"] == [(False, False), (True, True), (True, True), (False, True)]
    assert rag["fuse_c64"] == [(True, True)] and rag["fuse_c48_tw32"] == [(True, True)]
    assert rag["fuse_c48_tw24"] == [(True, False), (False, False)]  # (8 x 24 tiles need W % 24 == 0: rows only)
    # 96 channels: 4-row tiles and terms up to up = 2, which need H % 4 == 0 -- the support predicate leaves no ragged rows
    assert rag["fuse_c96_tw36"] == [(False, False)] and rag["fuse_c96_tw32"] == [(False, True)]
    f = fu.form(fu.EDGE_ROWS[2])  # 13 x 40: 8 + 5 rows, 16 + 16 + 8 columns
    assert (f.tiles_y, f.tiles_x, 13 % f.th, 40 % f.tile_w) == (2, 3, 5, 8)
    f = fu.form(next(r for r in fu.EDGE_ROWS if r.inst == "stem" and r.h == 20))  # out 5 x 17: 2 + 2 + 1 rows, 16 + 1 columns
    assert (f.tiles_y, f.tiles_x, 5 % f.th, 17 % f.tile_w) == (3, 2, 1, 1)


def test_later_tile_rows_exceed_what_the_device_holds_and_mix_the_images(lib):
    """Every LATE row has more tiles than workgroups can be resident on a device of up to CUS_SIZED_FOR compute units, and its batch -- a fixed
    pseudo-random sequence of the images A (2^-10) and B -- joins an A with a B in at least a quarter of the (tile, next tile of the same
    workgroup) pairs, for every grid mval_p2_walk_grid can answer: resident = 8, 16, ... up to the cap.  Pairs inside one image cannot join
    two images: a walk in steps of fewer tiles than an image has (resident < 8 tiles_img: a device of two or three compute units) is held to a
    quarter of its image-crossing pairs instead."""
    import ctypes

    grid = lib.mval_p2_walk_grid
    grid.restype, grid.argtypes = ctypes.c_int, [ctypes.c_int] * 3
    for r in fu.LATE_ROWS:
        f = fu.form(r)
        cap = pf.resident_cap(f, fu.CUS_SIZED_FOR)
        tiles_img = f.tiles_x * f.tiles_y
        assert f.tiles_total > cap and f.tiles_total == tiles_img * r.n and tiles_img > 1, fu.row_id(r)
        assert len(r.seq) == r.n and set(r.seq) == {"A", "B"} and r.seq == fu.late_seq(r.n)
        assert r.seq != ("AB" * r.n)[: r.n] and r.seq != ("BA" * r.n)[: r.n]
        assert fu.ragged(r, f) == ((False, True) if r.inst == "stem" else (True, True))  # (12 x 24: 8 + 4 rows, 16 + 8 columns; 6 x 20: 16 + 4 columns)
        worst = 1.0
        for resident in range(8, cap + 1, 8):
            wgs = grid(f.tiles_total, resident, 1)
            pairs = fu.walk_pairs(f.tiles_total, wgs)
            visits = walk(f.tiles_total, wgs)  # (the restated walk itself: the pairs are its consecutive visits of one workgroup)
            assert sorted(visits) == list(range(f.tiles_total)) and set(pairs) <= set(zip(visits, visits[1:])), (resident, wgs)
            assert len({b for _, b in pairs}) == len(pairs) and 0 < f.tiles_total - len(pairs) <= wgs, (resident, wgs)
            assert pairs, "some workgroup walks a second tile"
            step = pairs[0][1] - pairs[0][0]
            crossing = [(a, b) for a, b in pairs if a // tiles_img != b // tiles_img]
            mixed = sum(r.seq[a // tiles_img] != r.seq[b // tiles_img] for a, b in crossing)
            assert step >= tiles_img or resident < 8 * tiles_img
            of = len(pairs) if step >= tiles_img else len(crossing)
            worst = min(worst, mixed / of)
            assert 4 * mixed >= of, (fu.row_id(r), resident, wgs, mixed, len(crossing), len(pairs))
        print(f"[p2 fused] {fu.row_id(r)}: {f.tiles_total} tiles > {cap} resident; A-B pairs: at least {worst:.2f} of a walk's")


def test_fold_rows_have_more_tiles_per_image_than_slots():
    for r in fu.FOLD_ROWS:
        f = fu.form(r)
        assert f.tiles_x * f.tiles_y > fu.P2_SLOTS, fu.row_id(r)
        assert fu.factors(r) == fu.FOLD_FACTORS[: r.n]
    assert [r.n for r in fu.FOLD_ROWS if r.inst == "bneck_c64"] == [1]  # (its float64 reference is the expensive one)
    kind, shape, o, _ = fu.FOLD_CONV
    f = pf.query("op", *shape, kind, **pf.opts(o))
    assert f is not None and f.tiles_x * f.tiles_y * f.groups > fu.P2_SLOTS
    # (no row of tests/test_gpu_p2_forms.py reaches the fold: this one is not a repetition)
    import test_gpu_p2_forms as tf

    over = [tf._row_id(row) for row in tf.OP_CASES + tf.LATE_CASES for g in [tf._form(row)] if g.tiles_x * g.tiles_y * g.groups * g.parities > fu.P2_SLOTS]
    assert not over, over


def test_every_float64_reference_runs_on_the_cpu():
    """Every reference of the tables, once, with its time (the GPU tests compute them again: none may need more than about ten seconds)."""
    for r in fu.EDGE_ROWS + fu.LATE_ROWS + fu.FOLD_ROWS:
        t0 = time.perf_counter()
        t = fu.inputs(r)
        want = fu.want64(r, t)
        dt = time.perf_counter() - t0
        print(f"[p2 fused] {fu.row_id(r)}: float64 reference of {tuple(want.shape)} in {dt:.2f} s")
        assert want.shape == fu.out_shape(r, len(fu.factors(r))) and want.dtype == torch.float64 and bool(torch.isfinite(want).all())
        amax = want.abs().amax(dim=(1, 2, 3))
        assert bool((amax > 0).all()) and float(amax.max()) < 2.0 ** 20
        assert dt < 10.0, "shrink the row: its reference is too slow for the suite"


# ---- GPU ----
@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    from multi_view_active_learning_amd import _lib

    _lib.lib()
    return torch.device("cuda:0")


def _take(t, sel):
    """The images `sel` (a list of indices) of the tensors of fu.inputs."""
    pick = lambda v: None if v is None else v[sel].contiguous()
    return dict(x=pick(t["x"]), res=pick(t["res"]), convs=t["convs"], terms=[(pick(x), wt, sc, sh, up) for x, wt, sc, sh, up in t["terms"]])


def _build(r, t, dev):
    """The ops.P2Block / P2Bneck / P2Stem / P2FuseUp of the row on the tensors t."""
    from multi_view_active_learning_amd import ops

    nhwc = lambda v: None if v is None else v.permute(0, 2, 3, 1).contiguous().to(dev)
    kind = fu.kind_of(r)
    cv = [tuple(v.to(dev) for v in c) for c in t["convs"]]
    if kind == "block":
        return ops.P2Block(nhwc(t["x"]), *cv[0], *cv[1])
    if kind == "bneck":
        return ops.P2Bneck(nhwc(t["x"]), cv, nhwc(t["res"]))
    if kind == "stem":
        return ops.P2Stem(t["x"].to(dev), *cv[0], *cv[1])
    return ops.P2FuseUp(nhwc(t["res"]), [(nhwc(x), wt.to(dev), sc.to(dev), sh.to(dev), up) for x, wt, sc, sh, up in t["terms"]], relu=r.relu)


def _launch_checked(r, c, f, twice=False):
    """_launch_poisoned of tests/test_gpu_p2_forms.py for the four arena layouts (input planes | output planes | rows: inputs', then the output's;
    the stem: output planes | its in_row | out rows, the image outside).  Before the launch: the output region and its alignment padding, up to
    the first row, hold a NaN pattern, and the out rows' slots hold 2^20 -- slots [0, tiles_img) where every tile has a slot of its own, the
    WHOLE rows where the tiles fold (the launcher must zero them).  After it: every output fp16 is finite, the padding still holds the pattern,
    the input planes and the input / residual / term rows are bit-unchanged (the stem's in_row, written by its own launcher: the per-image
    max |x| of the image), the slots behind the tiles' -- folded: behind the P2_SLOTS -- are 0 and the scale slot is a power of two.  twice: a second launch on the same
    object leaves the same bits in the planes and in the rows."""
    n, ho, wo, cout = c.shape
    stem = fu.kind_of(r) == "stem"
    numel = n * ho * wo * cout
    rows_at = c.op.res1_amax_off if fu.kind_of(r) == "fuse" else c.op.in_amax_off  # the first row of the arena
    tiles_img = f.tiles_x * f.tiles_y
    fold = tiles_img > fu.P2_SLOTS
    bits = c.arena.view(torch.int32)
    assert 0 <= c.out_off and c.out_off + numel <= rows_at < c.op.out_amax_off and c.op.out_amax_off + n * fu.P2_ROW <= bits.numel()
    bits[c.out_off:rows_at] = NAN_BITS
    planes_in = (c.x if stem else bits[: c.out_off]).clone()
    rows_in = bits[rows_at:c.op.out_amax_off].clone()
    if fold:
        c.out_rows()[:] = BIG_BITS
    else:
        c.out_rows()[:, :tiles_img] = BIG_BITS
    c.launch()
    torch.cuda.synchronize()
    out = bits[c.out_off:c.out_off + numel]
    assert bool(torch.isfinite(out.view(torch.float16).float()).all()), "an output element was left unwritten or is not finite"
    assert bool((bits[c.out_off + numel:rows_at] == NAN_BITS).all()), "a store behind the output's last element"
    if stem:
        assert torch.equal(c.x, planes_in), "a store into the image"
        kept_in = bits[rows_at:c.op.out_amax_off].reshape(n, fu.P2_ROW)[:, : fu.P2_SLOTS].amax(1).view(torch.float32)
        assert torch.equal(kept_in, c.x.abs().amax(dim=(1, 2, 3))), "the stem's in_row: max |x| of each image"
    else:
        assert torch.equal(bits[: c.out_off], planes_in), "a store into the input planes"
        assert torch.equal(bits[rows_at:c.op.out_amax_off], rows_in), "a store into the input / residual / term rows"
    rows = c.out_rows()
    # (a row is P2_SLOTS partial maxima and the scale slot, csrc/conv_p2.h: nothing is kept behind the last tile's slot, nor -- folded -- behind
    # the slots, where the launcher's zeroes must have replaced the 2^20)
    assert bool((rows[:, min(tiles_img, fu.P2_SLOTS):fu.P2_INV_SLOT] == 0).all()), "a partial maximum behind the image's last slot"
    inv = rows[:, fu.P2_INV_SLOT]
    assert bool(((inv & 0x7FFFFF) == 0).all()) and bool((inv > 0).all()) and bool((inv < 0x7F800000).all()), "the scale slot holds a power of two"
    if twice:
        first, first_rows = out.clone(), rows.clone()
        c.launch()
        torch.cuda.synchronize()
        assert torch.equal(out, first), "a second launch on the same object gives other bits"
        assert torch.equal(c.out_rows(), first_rows), "a second launch on the same object leaves other rows"


def _run(r, t, dev, twice=False):
    """The row's launch on the tensors t -> (NCHW result, kept per-image maxima), on the CPU."""
    n = (t["x"] if t["x"] is not None else t["res"]).shape[0]
    f = fu.form(r, n)
    assert f is not None and fu.instance(r, f) == r.inst, "the case must run on the instance it is in the table for"
    c = _build(r, t, dev)
    _launch_checked(r, c, f, twice)
    return c.result().permute(0, 3, 1, 2).cpu(), c.kept_amax().cpu()


def _chain(r, t, dev):
    """The launches the fused one replaces, as the four older tests of tests/test_gpu_p2.py build them -> NCHW on the CPU."""
    from multi_view_active_learning_amd import ops

    nhwc = lambda v: v.permute(0, 2, 3, 1).contiguous().to(dev)
    kind = fu.kind_of(r)
    cv = [tuple(v.to(dev) for v in c) for c in t["convs"]]
    if kind == "block":
        xd = nhwc(t["x"])
        y = ops.fused_conv_p2(ops.fused_conv_p2(xd, *cv[0], relu=True), *cv[1], relu=True, res1=xd)
    elif kind == "bneck":
        xd = nhwc(t["x"])
        y = ops.fused_conv_p2(ops.fused_conv_p2(xd, *cv[0], relu=True), *cv[1], relu=True)
        y = ops.fused_conv_p2(y, *cv[2], relu=True, res1=xd if t["res"] is None else nhwc(t["res"]))
    elif kind == "stem":
        y = ops.fused_conv(t["x"].to(dev), *cv[0], stride=2, relu=True, algo=ops.ALGO_DIRECT, in_nchw=True)
        y = ops.fused_conv_p2(y, *cv[1], stride=2, relu=True)
    else:
        y = nhwc(t["res"])
        for j, (x, wt, sc, sh, up) in enumerate(t["terms"]):
            y = ops.fused_conv_p2(nhwc(x), wt.to(dev), sc.to(dev), sh.to(dev), relu=r.relu and j == len(t["terms"]) - 1, res1=y, up=up)
    return y.permute(0, 3, 1, 2).cpu()


def _assert_close(tag, got, want64, atol):
    """test_gpu_p2_forms._assert_close: elementwise against float64 at rtol 1e-4 and the launch's atol; prints the worst excess first."""
    w = want64.float()
    err = (got - w).abs()
    excess = float((err - (atol + RTOL * w.abs())).max())
    print(f"[p2 fused] {tag}: max |err| {float(err.max()):.3e}, max of |err| - (atol + rtol |want|) {excess:.3e}")
    assert got.shape == w.shape and bool(torch.isfinite(got).all()) and excess <= 0.0, (tag, float(err.max()), excess)


def _check_values(r, t, want, got, kept, dev):
    """(1) float64, (2) kept maxima, (3) not less accurate than the chain of launches it replaces: per image and over the batch."""
    tag = fu.row_id(r)
    _assert_close(tag, got, want, ATOL[fu.kind_of(r)])
    assert torch.allclose(kept, got.abs().amax(dim=(1, 2, 3)), rtol=2.0 ** -21, atol=0), ("kept per-image max |x|", kept, got.abs().amax(dim=(1, 2, 3)))
    n = got.shape[0]
    if want[0].numel() >= RMS_MIN_ELEMENTS and fu.chain_exists(r, n):
        chain = _chain(r, t, dev)
        rms = lambda y: (y.double() - want).pow(2).mean(dim=(1, 2, 3)).sqrt()
        rf, rc = rms(got), rms(chain)
        bf, bc = float(rf.pow(2).mean().sqrt()), float(rc.pow(2).mean().sqrt())
        rec = dict(images=[dict(factor=fu.factors(r)[i], fused=float(rf[i]), chain=float(rc[i]), ratio=float(rf[i] / rc[i])) for i in range(n)],
                   batch=dict(fused=bf, chain=bc, ratio=bf / bc))
        _RATIOS[tag] = rec
        _report("p2_fused_ratios.json", _RATIOS)
        print(f"[p2 fused] {tag}: rms / chain's per image " + ", ".join(f"{d['fused']:.3e} / {d['chain']:.3e} = {d['ratio']:.3f}" for d in rec["images"]) +
              f"; batch {bf:.3e} / {bc:.3e} = {bf / bc:.3f}")
        assert bf <= 1.25 * bc + 1e-8, ("batch", bf, bc)
        for i in range(n):
            assert float(rf[i]) <= 1.25 * float(rc[i]) + 1e-8, ("image", i, float(rf[i]), float(rc[i]))


def _check_alone(r, t, got, kept, dev):
    """(4) every image run alone (a batch of one) gives that image's bits and its kept maximum."""
    for i in range(got.shape[0]):
        alone, kept1 = _run(r, _take(t, [i]), dev)
        assert _bits_equal(alone[0], got[i]), f"image {i} alone has other bits"
        assert _bits_equal(kept1, kept[i : i + 1]), f"image {i} alone keeps another maximum"


@gpu
@pytest.mark.parametrize("r", fu.EDGE_ROWS, ids=fu.row_id)
def test_p2_fused_edges_vs_float64(dev, r):
    """Three images of magnitudes 2^-10, 2^-4 and 1 on the smallest maps that reach the instance's edges: (1) float64 at the bounds of
    tests/test_gpu_p2.py, (2) the kept maxima, (3) per image not less accurate than the chain, (4) every image alone gives its bits, (5) poison
    and (6) slots: _launch_checked."""
    t = fu.inputs(r)
    want = fu.want64(r, t)
    got, kept = _run(r, t, dev)
    _check_values(r, t, want, got, kept, dev)
    _check_alone(r, t, got, kept, dev)


@gpu
@pytest.mark.parametrize("r", fu.FOLD_ROWS, ids=fu.row_id)
def test_p2_fused_folded_maxima_vs_float64(dev, r):
    """More tiles per image than slots: the launcher zeroes the out rows (poisoned whole with 2^20 before) and the tiles fold their maxima with
    atomicMax; two launches on the same object give the same bits.  Otherwise as test_p2_fused_edges_vs_float64."""
    t = fu.inputs(r)
    want = fu.want64(r, t)
    got, kept = _run(r, t, dev, twice=True)
    _check_values(r, t, want, got, kept, dev)
    _check_alone(r, t, got, kept, dev)


@gpu
def test_p2_conv_folded_maxima_vs_float64(dev):
    """The same fold in the single conv (ops.P2Conv: a 3x3 conv c32 -> c32 on 136 x 256, tiles_x * tiles_y * groups > 256), the second image
    scaled 2^-10: float64, kept maxima, whole out rows poisoned, two launches."""
    import test_gpu_p2_forms as tf
    from multi_view_active_learning_amd import ops

    kind, shape, o, _ = row = fu.FOLD_CONV
    f = pf.query("op", *shape, kind, **pf.opts(o))
    assert f.tiles_x * f.tiles_y * f.groups > fu.P2_SLOTS
    t = tf._inputs(row)
    t[0][1] *= fu.FOLD_FACTORS[1]
    want = tf._want64(row, t)
    x, wt, scale, shift, _, _ = t
    c = ops.P2Conv(x.permute(0, 2, 3, 1).contiguous().to(dev), wt.to(dev), scale.to(dev), shift.to(dev), relu=True)
    c.out_rows()[:] = BIG_BITS
    _launch_poisoned(c)
    got, kept, rows = c.result().permute(0, 3, 1, 2).cpu(), c.kept_amax().cpu(), c.out_rows().clone()
    _assert_close("conv_c32-32_n2_136x256_k3s1", got, want, 2e-5)
    assert bool((rows[:, fu.P2_SLOTS:fu.P2_INV_SLOT] == 0).all()), "a partial maximum behind the image's last slot"
    assert torch.allclose(kept, got.abs().amax(dim=(1, 2, 3)), rtol=2.0 ** -21, atol=0), "kept per-image max |x|"
    c.launch()
    torch.cuda.synchronize()
    assert _bits_equal(c.result().permute(0, 3, 1, 2).cpu(), got) and torch.equal(c.out_rows(), rows), "a second launch gives other bits"


@gpu
@pytest.mark.parametrize("r", fu.LATE_ROWS, ids=fu.row_id)
def test_p2_fused_later_tiles_of_a_workgroup(dev, r):
    """A batch of the images A (2^-10) and B in a pseudo-random order, so large that some workgroup must walk two tiles or more (asserted from the
    device's compute units).  The first A and the first B as in test_p2_fused_edges_vs_float64; every other image equals its kind's first
    occurrence bit for bit, its kept maximum too: what a workgroup carries from tile to tile -- the prefetched next patch, the chunks staged by
    the tile before, the scales, the partial maxima -- leaves no trace in the results."""
    f = fu.form(r)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    cap = pf.resident_cap(f, cus)
    print(f"[p2 fused] {fu.row_id(r)}: {f.tiles_total} tiles, at most {cap} resident workgroups on {cus} compute units")
    assert f.tiles_total > cap, (f.tiles_total, cus, cap)
    two = fu.inputs(r)
    want = fu.want64(r, two)
    idx = ["AB".index(ch) for ch in r.seq]
    got, kept = _run(r, _take(two, idx), dev)
    first = [idx.index(0), idx.index(1)]
    _check_values(r, two, want, got[first], kept[first], dev)
    same = torch.tensor([first[k] for k in idx])
    assert _bits_equal(got, got[same]), "an image differs from the first one of its kind"
    assert _bits_equal(kept, kept[same]), "a kept maximum differs from the first one of its kind"
    _check_alone(r, two, got[first], kept[first], dev)
