"""GPU tests of the flip test: ``mval_mirror_images`` and ``mval_flip_merge_heatmaps`` against the numpy float32
oracle of tests/flip_oracle.py, bit for bit -- values, arg-max keys, independence from the rest of the batch, argument checks -- and
the calls that carry the stage: ``_compute_batch_heatmap_flip``, the scoring pass and the evaluation on a small synthetic HRNet."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))

import cases  # noqa: E402
import flip_oracle as fo  # noqa: E402
from multi_view_active_learning_amd import synth  # noqa: E402

pytestmark = pytest.mark.gpu

MIRROR_SHAPES = [(7, 1), (5, 3), (6, 64), (4, 72), (2, 257)]
# (N, J, hh, wh): one pixel; one column (the shift on a one-column map); odd and smaller than a wave; a loop over the workgroup
# with wh no multiple of 64; the largest map of the project's configs
MERGE_SHAPES = [(2, 4, 1, 1), (2, 3, 3, 1), (3, 5, 5, 7), (2, 19, 64, 48), (1, 42, 96, 72)]
MODES = ("mirror", "mirror_shift")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from multi_view_active_learning_amd import _lib

    _lib.lib()  # fail loudly when the extension is missing
    return torch.device("cuda:0")


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _pairs_for(j):
    """A table that mixes swapped and self-paired channels: (i, j-1-i) swapped for even i, the rest their own twin."""
    table = list(range(j))
    for i in range(0, j // 2, 2):
        table[i], table[j - 1 - i] = j - 1 - i, i
    return table


_CASES = {}


def _case(shape):
    """The inputs of a merge case, made once: normal draws (|v| >= 1e-30 or exactly 0), and four planted maps -- map m = n * J + j is
    fed by hm[n, j] and hm_mirrored[n, pairs[j]] alone, so each plant reaches one merged map:
      map 0       the maximum twice (not on a one-pixel map)          map 1       a NaN, from either input
      last map    all zero with a -0 (arg-max 0)                      last but one  all -inf (arg-max 0)"""
    if shape in _CASES:
        return _CASES[shape]
    n, j, hh, wh = shape
    npix = hh * wh
    rng = np.random.default_rng(1000 + n * j * npix)
    pairs = _pairs_for(j)
    hm, hmm = (rng.standard_normal(shape).astype(np.float32) for _ in range(2))
    for a in (hm, hmm):
        a[np.abs(a) < 1e-30] = 0.0
        a[rng.uniform(size=shape) < 0.02] = 0.0

    def maps(m):  # (the map of hm and the map of hm_mirrored that feed merged map m, as flat views)
        return hm[m // j, m % j].reshape(-1), hmm[m // j, pairs[m % j]].reshape(-1)

    a, b = maps(0)
    if npix >= 2:
        b[:] = 0.0
        a[[npix // 3, npix - 1]] = 16.0
    a, b = maps(1)
    a[min(1, npix - 1)] = np.nan
    b[npix // 2] = np.nan
    a, b = maps(n * j - 1)
    a[:], b[:] = 0.0, -0.0
    a[npix - 1] = -0.0
    a, b = maps(n * j - 2)
    a[:], b[:] = -np.inf, -np.inf
    want = {mode: fo.merge(hm, hmm, pairs, mode == "mirror_shift") for mode in MODES}
    for w in want.values():  # the plants are what they say
        flat = w.reshape(n * j, npix)
        if npix >= 2:
            assert flat[0].max() == 8.0 and (flat[0] == 8.0).sum() == 2
        assert np.isnan(flat[1]).any()
        assert not flat[-1].any() and np.signbit(flat[-1]).any() and np.isneginf(flat[-2]).all()
    first = {mode: np.array([fo.first_argmax(m) for m in w.reshape(n * j, npix)]).reshape(n, j) for mode, w in want.items()}
    _CASES[shape] = dict(hm=hm, hmm=hmm, pairs=pairs, want=want, first=first)
    return _CASES[shape]


def _merge(dev, c, mode, **kw):
    from multi_view_active_learning_amd import _lib

    pairs = torch.tensor(c["pairs"], dtype=torch.int32, device=dev)
    return _lib.flip_merge_heatmaps(torch.from_numpy(c["hm"]).to(dev), torch.from_numpy(c["hmm"]).to(dev), pairs, mode == "mirror_shift", **kw)


# ---- 1. the mirror -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows, w", MIRROR_SHAPES)
def test_mirror_images_bit_copy(dev, rows, w):
    """Every bit pattern comes through (NaN payloads, -0, subnormals): the input is random 32-bit words."""
    from multi_view_active_learning_amd import _lib

    words = np.random.default_rng(rows * 1000 + w).integers(-(1 << 31), 1 << 31, size=(rows, w), dtype=np.int64).astype(np.int32)
    x = torch.from_numpy(words.view(np.float32)).to(dev)
    got = _lib.mirror_images(x)
    assert got.shape == x.shape and got.dtype == torch.float32
    np.testing.assert_array_equal(_bits(got.cpu().numpy()), _bits(fo.mirror(words.view(np.float32))))
    x4 = x.reshape(1, rows, 1, w)  # (any leading shape: the rows are what counts)
    np.testing.assert_array_equal(_bits(_lib.mirror_images(x4).cpu().numpy()), _bits(fo.mirror(words.view(np.float32)).reshape(1, rows, 1, w)))
    np.testing.assert_array_equal(_bits(x.cpu().numpy()), words)  # the input is untouched


# ---- 2. the merge, 3. its keys ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", MERGE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_flip_merge_values_and_keys(dev, shape, mode):
    """The merged maps equal the oracle's bit for bit; the emitted keys decode to the arg-max of the merged maps -- the device's
    own second read and the oracle's first_argmax, the planted maps included --, their unused slots are 0 and they are remembered
    for the merged tensor."""
    from multi_view_active_learning_amd import _lib

    n, j, hh, wh = shape
    c = _case(shape)
    got = _merge(dev, c, mode)
    assert got.shape == shape and got.dtype == torch.float32 and got.is_contiguous()
    np.testing.assert_array_equal(_bits(got.cpu().numpy()), _bits(c["want"][mode]))
    keys = _lib.argmax_keys_of(got)
    assert keys is not None and tuple(keys.shape) == (n, _lib.ARGMAX_SLOTS, j) and keys.dtype == torch.int64
    assert _lib.argmax_keys_of(got.reshape(n, 1, j, hh, wh)) is keys  # (any full reshape, as for a network output)
    assert not bool(keys[:, 4:, :].any().item())  # one slot per wave: 4 of them
    assert bool((keys[:, :4, :] != 0).any(dim=1).all().item())  # every map has a key
    from_keys = _lib.argmax_from_keys(keys, None, n, 1, j, 1, wh).cpu().numpy().reshape(n, j, 2)
    plain = got.clone()  # (no keys remembered for the copy: the decode reads the maps)
    assert _lib.argmax_keys_of(plain) is None
    from_maps = _lib.argmax_decode(plain, None, n, 1, j, hh, wh, 1, wh).cpu().numpy().reshape(n, j, 2)
    np.testing.assert_array_equal(from_keys, from_maps)
    np.testing.assert_array_equal(from_keys[..., 1] * wh + from_keys[..., 0], c["first"][mode])
    np.testing.assert_array_equal(_lib.argmax_decode(got, None, n, 1, j, hh, wh, 1, wh).cpu().numpy().reshape(n, j, 2), from_maps)  # (the keys' path)
    flat = c["first"][mode].reshape(-1)
    assert flat[-1] == 0 and flat[-2] == 0 and (hh * wh < 2 or flat[0] == hh * wh // 3)


def test_keep_keys_false_remembers_nothing(dev):
    from multi_view_active_learning_amd import _lib

    c = _case(MERGE_SHAPES[2])
    got = _merge(dev, c, "mirror", keep_keys=False)
    assert _lib.argmax_keys_of(got) is None
    np.testing.assert_array_equal(_bits(got.cpu().numpy()), _bits(c["want"]["mirror"]))
    # a tensor handed in as ``out``: its keys are those of the last launch that wrote it, never an earlier one's
    kept = _merge(dev, c, "mirror")
    first = _lib.argmax_keys_of(kept)
    assert _merge(dev, c, "mirror_shift", out=kept) is kept
    second = _lib.argmax_keys_of(kept)
    assert second is not None and second is not first
    n, j, hh, wh = MERGE_SHAPES[2]
    xy = _lib.argmax_from_keys(second, None, n, 1, j, 1, wh).cpu().numpy().reshape(n, j, 2)
    np.testing.assert_array_equal(xy[..., 1] * wh + xy[..., 0], c["first"]["mirror_shift"])
    assert _merge(dev, c, "mirror", keep_keys=False, out=kept) is kept and _lib.argmax_keys_of(kept) is None
    kept = _merge(dev, c, "mirror")
    _lib.mirror_images(torch.from_numpy(c["hm"]).to(dev), out=kept)  # (any launch of the package that writes into it)
    assert _lib.argmax_keys_of(kept) is None


def test_merge_flipped_checks_pairs_and_caches_them(dev):
    from multi_view_active_learning_amd.utils import flip_test

    c = _case(MERGE_SHAPES[2])
    hm, hmm = torch.from_numpy(c["hm"]).to(dev), torch.from_numpy(c["hmm"]).to(dev)
    for mode in MODES:
        np.testing.assert_array_equal(_bits(flip_test.merge_flipped(hm, hmm, c["pairs"], mode).cpu().numpy()), _bits(c["want"][mode]))
    assert flip_test.pairs_on_device(c["pairs"], dev) is flip_test.pairs_on_device(tuple(c["pairs"]), torch.device("cuda", 0))
    with pytest.raises(ValueError, match="own inverse"):
        flip_test.merge_flipped(hm, hmm, [1, 2, 0, 3, 4], "mirror")
    with pytest.raises(ValueError, match="4 entries for 5 joints"):
        flip_test.merge_flipped(hm, hmm, [1, 0, 2, 3], "mirror")


# ---- 4. a map alone --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", [MERGE_SHAPES[2], MERGE_SHAPES[3]], ids=lambda s: "x".join(map(str, s)))
def test_self_paired_map_alone(dev, shape, mode):
    """A self-paired map run as N = J = 1 gives the bits and the arg-max it gives inside its batch."""
    from multi_view_active_learning_amd import _lib

    c = _case(shape)
    j = next(i for i, p in enumerate(c["pairs"]) if p == i)
    n = shape[0] - 1
    hm, hmm = (torch.from_numpy(np.ascontiguousarray(c[k][n : n + 1, j : j + 1])).to(dev) for k in ("hm", "hmm"))
    got = _lib.flip_merge_heatmaps(hm, hmm, torch.zeros(1, dtype=torch.int32, device=dev), mode == "mirror_shift")
    np.testing.assert_array_equal(_bits(got.cpu().numpy()), _bits(c["want"][mode][n : n + 1, j : j + 1]))
    xy = _lib.argmax_from_keys(_lib.argmax_keys_of(got), None, 1, 1, 1, 1, shape[3]).cpu().numpy().reshape(2)
    assert xy[1] * shape[3] + xy[0] == c["first"][mode][n, j]


# ---- 5. argument checks ----------------------------------------------------------------------------------------------------------
def test_wrappers_refuse_and_take_empty_batches(dev):
    from multi_view_active_learning_amd import _lib

    hm, hmm = torch.zeros(2, 3, 4, 5, device=dev), torch.ones(2, 3, 4, 5, device=dev)
    pairs = torch.tensor([2, 1, 0], dtype=torch.int32, device=dev)
    for out in (hm, hmm):
        with pytest.raises(_lib.MvalError, match="alias"):
            _lib.flip_merge_heatmaps(hm, hmm, pairs, 0, out=out)
    x = torch.zeros(4, 6, device=dev)
    with pytest.raises(_lib.MvalError, match="alias"):
        _lib.mirror_images(x, out=x)
    with pytest.raises(_lib.MvalError, match="bad dims"):  # J = 0
        _lib.flip_merge_heatmaps(torch.zeros(2, 0, 4, 5, device=dev), torch.zeros(2, 0, 4, 5, device=dev), pairs[:0], 0)
    with pytest.raises(_lib.MvalError, match="one shape"):
        _lib.flip_merge_heatmaps(hm, hmm[:, :, :, :4].contiguous(), pairs, 0)
    with pytest.raises(_lib.MvalError, match="one shape"):
        _lib.flip_merge_heatmaps(hm[0], hmm[0], pairs, 0)
    with pytest.raises(_lib.MvalError, match=r"pairs must be \(3,\)"):
        _lib.flip_merge_heatmaps(hm, hmm, pairs[:2], 0)
    with pytest.raises(_lib.MvalError, match="expected torch.int32"):
        _lib.flip_merge_heatmaps(hm, hmm, pairs.to(torch.int64), 0)
    with pytest.raises(_lib.MvalError, match="out must be"):
        _lib.flip_merge_heatmaps(hm, hmm, pairs, 0, out=torch.zeros(2, 3, 4, 4, device=dev))
    with pytest.raises(_lib.MvalError, match="a view of"):  # (the keys are remembered per base tensor)
        _lib.flip_merge_heatmaps(hm, hmm, pairs, 0, out=torch.zeros(4, 3, 4, 5, device=dev)[:2])
    torch.cuda.synchronize()
    assert bool((hm == 0).all().item()) and bool((hmm == 1).all().item())  # nothing was launched on them
    empty = _lib.flip_merge_heatmaps(hm[:0], hmm[:0], pairs, 1)
    assert tuple(empty.shape) == (0, 3, 4, 5) and tuple(_lib.argmax_keys_of(empty).shape) == (0, _lib.ARGMAX_SLOTS, 3)
    assert tuple(_lib.mirror_images(x[:0]).shape) == (0, 6)


# ---- 6. end to end ---------------------------------------------------------------------------------------------------------------
B, V = 2, 2
E2E_PAIRS = [[0, 4], [1, 3]]  # of the five joints of the small HRNet case; joint 2 is its own twin
TABLE = [4, 3, 2, 1, 0]


@pytest.fixture(scope="module")
def net(dev):
    """The smallest synthetic HRNet of the model cases (w32_small: five joints, 64 x 96 input, 16 x 24 maps) on a batch of
    B = 2 frames x V = 2 views, as float32 and as a uint8 compact batch, with the network's maps of each batch and of its mirror
    image -- computed once and left unchanged."""
    from multi_view_active_learning_amd.utils import preprocess

    c = cases.model_cases()["w32_small"]
    m = cases.product_model(c)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in cases.model_state_dict(c).items()}, strict=True)
    m = m.to(dev).eval()
    h, w, j = c["h"], c["w"], c["j"]
    f32 = synth.images(c["seed"] + 50, B, V, h, w)
    u8 = np.random.default_rng(c["seed"] + 51).integers(0, 256, size=(B, V, h, w, 3), dtype=np.uint8)
    out = dict(model=m, j=j, h=h, w=w, f32=f32, u8=u8, maps={})
    with torch.no_grad():
        u8_as_f32 = preprocess.normalize_views_u8(torch.from_numpy(u8).to(dev).reshape(-1, h, w, 3)).cpu().numpy()
        for kind, x in (("f32", f32.reshape(B * V, 3, h, w)), ("u8", u8_as_f32)):
            a = m(torch.from_numpy(x).to(dev)).cpu().numpy()
            b = m(torch.from_numpy(fo.mirror(x)).to(dev)).cpu().numpy()
            assert a.shape == (B * V, j, h // 4, w // 4)
            out["maps"][kind] = (a, b)
    return out


def _cfg(j):
    from multi_view_active_learning_amd.config import get_default_configs

    cfg = get_default_configs()
    cfg.DATA.NUM_JOINTS, cfg.DATA.FLIP_PAIRS, cfg.POSE_ESTIMATOR.STRIDE = j, E2E_PAIRS, 4
    cfg.AL.STRATEGY = "TRIANGULATION"
    return cfg


@pytest.mark.parametrize("kind", ["f32", "u8"])
@pytest.mark.parametrize("mode", MODES)
def test_compute_batch_heatmap_flip(dev, net, mode, kind):
    """``_compute_batch_heatmap_flip`` is the oracle's merge of model(x) and model(mirror(x)), bit for bit, for a float32 batch and a
    uint8 compact one (normalised once; the float32 result is what is mirrored), and the result carries its keys."""
    from multi_view_active_learning_amd import _lib
    from multi_view_active_learning_amd.strategy import ActiveLearningStrategy

    st = ActiveLearningStrategy(_cfg(net["j"]))
    with torch.no_grad():
        got = st._compute_batch_heatmap_flip(net["model"], {"images": torch.from_numpy(net[kind])}, mode)
    want = fo.merge(*net["maps"][kind], TABLE, mode == "mirror_shift")
    np.testing.assert_array_equal(_bits(got.cpu().numpy()), _bits(want))
    assert _lib.argmax_keys_of(got) is not None
    assert not np.array_equal(_bits(want), _bits(net["maps"][kind][0]))  # (the second forward matters on this input)


def test_mirrored_batch_gives_mirrored_swapped_maps(dev, net):
    """Under "mirror" the merged maps of the mirrored batch are the mirrored, pair-swapped merged maps of the batch, bit for bit:
    a wrong pair table or column index breaks it."""
    from multi_view_active_learning_amd.strategy import ActiveLearningStrategy

    st = ActiveLearningStrategy(_cfg(net["j"]))
    with torch.no_grad():
        fwd = st._compute_batch_heatmap_flip(net["model"], {"images": torch.from_numpy(net["f32"])}, "mirror").cpu().numpy()
        back = st._compute_batch_heatmap_flip(net["model"], {"images": torch.from_numpy(fo.mirror(net["f32"]))}, "mirror").cpu().numpy()
    np.testing.assert_array_equal(_bits(back), _bits(fo.mirror(fwd[:, TABLE])))
    assert not np.array_equal(_bits(back), _bits(fo.mirror(fwd)))  # (the swap matters on this input)


def _loader(net):
    j, h, w = net["j"], net["h"], net["w"]
    proj = np.stack([synth.ring_cameras(V, h, w, seed=s) for s in range(B)])
    gt = np.concatenate([synth.joints_3d(3, B, j), np.ones((B, 1, j), dtype=np.float32)], axis=1)
    valid = np.ones((B, j), dtype=np.float32)
    valid[1, 3] = 0
    dp = dict(images=net["f32"], pose=np.arange(B, dtype=np.int64) + 7, frame_id=np.arange(B, dtype=np.int64) * 3, proj_matrices=proj,
              joint_valid=valid, **{"3d_keypoints": gt})
    return [{k: torch.from_numpy(a) for k, a in dp.items()}]


def _same_bits(a, b):
    as_int = torch.int64 if a.dtype == torch.float64 else torch.int32
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(as_int), b.contiguous().view(as_int))


def test_evaluate_mkpe_under_flip_test(dev, net):
    """evaluate_mkpe under EVAL.FLIP_TEST = "mirror_shift" is the MKPE of triangulate_batch on the oracle-merged maps; AL.FLIP_TEST
    has no say in it."""
    from multi_view_active_learning_amd import _lib
    from multi_view_active_learning_amd.strategy import ActiveLearningStrategy
    from multi_view_active_learning_amd.utils.triangulation import triangulate_batch

    j = net["j"]
    cfg = _cfg(j)
    cfg.AL.FLIP_TEST = "mirror"
    loader = _loader(net)
    plain = ActiveLearningStrategy(cfg).evaluate_mkpe(loader, net["model"])
    cfg.EVAL.FLIP_TEST = "mirror_shift"
    st = ActiveLearningStrategy(cfg)
    got = st.evaluate_mkpe(loader, net["model"])
    dp = loader[0]
    hm = torch.from_numpy(fo.merge(*net["maps"]["f32"], TABLE, True)).to(dev)
    jv = dp["joint_valid"].reshape(B, j)
    r = triangulate_batch(hm.reshape(B, V, j, *hm.shape[2:]), dp["proj_matrices"], 4, jv)
    pred = r["keypoints_3d"].to(torch.float32)
    want, _ = _lib.mkpe(pred.contiguous(), dp["3d_keypoints"].to(dev, torch.float32).contiguous(), jv.to(dev, torch.float32).contiguous(), B, j, 4)
    assert _same_bits(got, want) and _same_bits(st._eval_tables[0], pred)
    hm0 = torch.from_numpy(net["maps"]["f32"][0]).to(dev)
    r0 = triangulate_batch(hm0.reshape(B, V, j, *hm0.shape[2:]), dp["proj_matrices"], 4, jv)
    want0, _ = _lib.mkpe(r0["keypoints_3d"].to(torch.float32).contiguous(), dp["3d_keypoints"].to(dev, torch.float32).contiguous(),
                         jv.to(dev, torch.float32).contiguous(), B, j, 4)
    assert _same_bits(plain, want0)  # ("none": one forward, as ever)
    print("evaluate_mkpe on synthetic weights (no accuracy figure): none %r, mirror_shift %r" % (float(plain.item()), float(got.item())))


def test_sal_dict_under_flip_test(dev, net):
    """_compute_sal_dict under AL.FLIP_TEST = "mirror" is tables_to_sal_dict of score_batch on the oracle-merged maps; EVAL.FLIP_TEST
    has no say in it."""
    from multi_view_active_learning_amd.strategy import ActiveLearningStrategy, tables_to_sal_dict

    cfg = _cfg(net["j"])
    cfg.EVAL.FLIP_TEST = "mirror_shift"
    cfg.AL.FLIP_TEST = "mirror"
    loader = _loader(net)
    got = ActiveLearningStrategy(cfg)._compute_sal_dict(loader, net["model"])
    st = ActiveLearningStrategy(cfg)
    st._pending_checks = []
    hm = torch.from_numpy(fo.merge(*net["maps"]["f32"], TABLE, False)).to(dev)
    table = st.score_batch(hm, st._stage_masked(loader[0]))
    want = tables_to_sal_dict([table.cpu().numpy()], [B])
    assert list(got) == list(want) and len(got["al_metric"]) == B
    for k in want:
        assert list(got[k]) == list(want[k]), k
        for guid in want[k]:
            np.testing.assert_array_equal(np.asarray(got[k][guid], dtype=np.float64).view(np.int64),
                                          np.asarray(want[k][guid], dtype=np.float64).view(np.int64), err_msg="%s %s" % (k, guid))


def test_none_never_enters_the_flip_path(dev, net, monkeypatch):
    """Under "none" a scoring pass and an evaluation pass never enter ``_compute_batch_heatmap_flip`` nor launch the two entries."""
    from multi_view_active_learning_amd import _lib
    from multi_view_active_learning_amd.strategy import ActiveLearningStrategy

    cfg = _cfg(net["j"])
    st = ActiveLearningStrategy(cfg)
    monkeypatch.setattr(ActiveLearningStrategy, "_compute_batch_heatmap_flip", lambda *a, **k: pytest.fail("the default configuration must not flip"))
    monkeypatch.setattr(_lib, "mirror_images", lambda *a, **k: pytest.fail("the default configuration must not mirror"))
    monkeypatch.setattr(_lib, "flip_merge_heatmaps", lambda *a, **k: pytest.fail("the default configuration must not merge"))
    loader = _loader(net)
    assert len(st._compute_sal_dict(loader, net["model"])["al_metric"]) == B
    assert st.evaluate_mkpe(loader, net["model"]).numel() == 1
