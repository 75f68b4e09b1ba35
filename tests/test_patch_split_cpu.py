"""CPU: the host side of the patch-wise mode (`split_input_params`) -- the blend weights against the reference's recorded
`weighting` / `normalization` (tests/golden/g19_split.npz, tools/make_golden_split.py), the geometries that are refused, and
the argument validation of the two kernels' entry points (it precedes any launch)."""
import numpy as np
import pytest
import torch

from conftest import golden

SPLIT = dict(ks=(32, 32), stride=(16, 16), vqf=4, patch_distributed_vq=True, tie_braker=False, clip_min_weight=0.01,
             clip_max_weight=0.5, clip_min_tie_weight=0.01, clip_max_tie_weight=0.5)


def geom(shape, ks=None, stride=None, uf=1, df=1, **over):
    from dsml_thesis_amd.patches import patch_geometry
    p = dict(SPLIT, **over)
    return patch_geometry(shape, ks or p["ks"], stride or p["stride"], uf=uf, df=df, params=p)


@pytest.mark.parametrize("tag,shape,kw,want", [("", (48, 64), {}, (2, 3)), ("_dec", (48, 64), dict(uf=4), (2, 3)),
                                               ("_enc", (192, 256), dict(df=4), (11, 15))])
def test_geometry_equals_the_reference_bit_for_bit(tag, shape, kw, want):
    g = golden("g19_split.npz")
    ly, lx, weight, norm = geom(shape, **kw)
    assert (ly, lx) == want
    assert weight.dtype == torch.float32 and norm.dtype == torch.float32
    assert np.array_equal(weight.numpy(), g["weight" + tag]), "weight"
    assert np.array_equal(norm.numpy(), g["norm" + tag]), "norm"


def test_tie_breaker_geometry_equals_the_reference_bit_for_bit():
    g = golden("g19_split.npz")
    ly, lx, weight, norm = geom((16, 16), (8, 8), (4, 4), tie_braker=True)
    assert (ly, lx) == (3, 3) and tuple(weight.shape) == (8, 8, 9)
    assert np.array_equal(weight.numpy(), g["weight_tie"]) and np.array_equal(norm.numpy(), g["norm_tie"])
    # the tie-breaker changes the weights: the two settings are not confused by the cache
    _, _, plain, _ = geom((16, 16), (8, 8), (4, 4))
    assert not torch.equal(plain, weight)


def test_geometry_is_cached():
    a, b = geom((48, 64)), geom((48, 64))
    assert a[2] is b[2] and a[3] is b[3]


def test_ks_and_stride_shrink_to_the_input():
    from dsml_thesis_amd.patches import reduce_ks_stride
    assert reduce_ks_stride((16, 24), (32, 32), (20, 30)) == ((16, 24), (16, 24))
    assert reduce_ks_stride((16, 24), (8, 32), (4, 4)) == ((8, 24), (4, 4))         # (both sides are clamped as soon as one is too large)
    assert reduce_ks_stride((48, 64), (32, 32), (16, 16)) == ((32, 32), (16, 16))
    ly, lx, weight, norm = geom((16, 24), (32, 32), (20, 30))
    ly2, lx2, weight2, norm2 = geom((16, 24), (16, 24), (16, 24))
    assert (ly, lx) == (ly2, lx2) == (1, 1) and tuple(weight.shape) == (16, 24, 1)
    assert torch.equal(weight, weight2) and torch.equal(norm, norm2)
    assert torch.equal(norm, weight[:, :, 0])                                       # one patch: the accumulated weight is the weight


@pytest.mark.parametrize("what,args,kw,match", [
    ("uncovered rows / columns", ((50, 64),), {}, "do not cover"),
    ("uncovered after the stride", ((48, 64), (32, 32), (12, 16)), {}, "do not cover"),
    ("kh == 1", ((4, 8), (1, 4), (1, 4)), {}, "divides by"),
    ("kw == 1", ((8, 4), (4, 1), (4, 1)), {}, "divides by"),
    ("tie-breaker with one row of patches", ((8, 16), (8, 8), (4, 4)), dict(tie_braker=True), "tie_braker"),
    ("tie-breaker with one column of patches", ((16, 8), (8, 8), (4, 4)), dict(tie_braker=True), "tie_braker"),
    ("non-square ks with vqf (decode)", ((48, 64), (32, 16), (16, 16)), dict(uf=4), "non-square"),
    ("non-square ks with vqf (encode)", ((192, 256), (32, 64), (16, 16)), dict(df=4), "non-square"),
])
def test_geometries_the_reference_turns_into_nan_or_a_shape_error_are_refused(what, args, kw, match):
    with pytest.raises(ValueError, match=match):
        geom(*args, **kw)


def test_delta_border_is_the_reference_formula():
    """min over the four normalised border distances (ddpm.py:572-584): 0 on the border, symmetric, at most 0.5."""
    from dsml_thesis_amd.patches import delta_border
    d = delta_border(5, 9)
    assert d.dtype == torch.float32 and tuple(d.shape) == (5, 9)
    assert float(d[0].max()) == 0 and float(d[:, 0].max()) == 0 and float(d[-1].max()) == 0 and float(d[:, -1].max()) == 0
    assert torch.equal(d, d.flip(0)) and float(d[2, 4]) == 0.5
    assert float(d[1, 1]) == pytest.approx(1 / 8) and float(d[2, 2]) == pytest.approx(2 / 8)


@pytest.fixture(scope="module")
def lib():
    from dsml_thesis_amd.build import build_lib
    build_lib(verbose=False)
    from dsml_thesis_amd import lib as L
    return L.load()


P = 4096    # never dereferenced: validation precedes any launch


def test_entry_points_validate_without_a_gpu(lib):
    ok = (2, 3, 48, 64, 32, 32, 16, 16, 2, 3)

    def both(geo):
        return (lib.ldmk_patch_unfold(P, P, *geo, None), lib.ldmk_patch_fold(P, P, P, P, *geo, None))

    # null pointers
    assert lib.ldmk_patch_unfold(0, P, *ok, None) == -1 and b"null pointer" in lib.ldmk_last_error()
    assert lib.ldmk_patch_unfold(P, 0, *ok, None) == -1 and b"null pointer" in lib.ldmk_last_error()
    for k in range(4):
        ptrs = [P] * 4
        ptrs[k] = 0
        assert lib.ldmk_patch_fold(*ptrs, *ok, None) == -1 and b"ldmk_patch_fold: null pointer" in lib.ldmk_last_error()
    # non-positive sizes
    for k in range(10):
        bad = list(ok)
        bad[k] = 0
        assert both(bad) == (-1, -1) and b"must be positive" in lib.ldmk_last_error(), k
    # patch larger than the image
    assert both((1, 3, 16, 64, 32, 32, 16, 16, 1, 3)) == (-1, -1) and b"larger than the image" in lib.ldmk_last_error()
    assert both((1, 3, 48, 16, 32, 32, 16, 16, 2, 1)) == (-1, -1) and b"larger than the image" in lib.ldmk_last_error()
    # ly / lx that are not the patch counts of the geometry (a transposed pair among them)
    assert both((2, 3, 48, 64, 32, 32, 16, 16, 3, 2)) == (-1, -1) and b"ly=3 lx=2" in lib.ldmk_last_error()
    assert both((2, 3, 48, 64, 32, 32, 16, 16, 2, 2)) == (-1, -1)
    # patches that do not tile the image: the last rows / columns would be 0/0
    assert both((2, 3, 50, 64, 32, 32, 16, 16, 2, 3)) == (-1, -1) and b"do not cover" in lib.ldmk_last_error()
    assert both((2, 3, 48, 66, 32, 32, 16, 16, 2, 3)) == (-1, -1) and b"do not cover" in lib.ldmk_last_error()


def test_wrapper_raises_with_the_library_message(lib):
    from dsml_thesis_amd import lib as L
    with pytest.raises(L.LdmkError, match="do not cover"):
        L.call("ldmk_patch_unfold", P, P, 2, 3, 50, 64, 32, 32, 16, 16, 2, 3, None)
