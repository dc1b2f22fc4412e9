"""Large-steps preconditioning (hf_large_steps_*) on the CPU: the entry points are declared, exported and bound; every bad
argument is refused with HF_EINVAL before anything touches a device (host addresses stand in for device pointers, so a
call that got as far as a launch would not return HF_EINVAL); HF_VERSION is unchanged."""
import pytest

from abi_helpers import assert_refused, assert_symbols, stand_ins

FNS = ("hf_large_steps_workspace_floats", "hf_large_steps_apply", "hf_large_steps_solve")
NAN, INF = float("nan"), float("inf")


def test_symbols_declared_exported_and_bound():
    assert_symbols(FNS, ("LargeSteps",))


def test_workspace_size():
    """four vectors of W H floats (rounded up to 16 bytes), four rows of 16384 fp64 partials (the cap of the flat grid
    family), four fp64 scalars and four words"""
    from hf_amd import _capi
    f = _capi.lib().hf_large_steps_workspace_floats
    tail = 2 * (4 * 16384 + 4) + 4
    assert f(2, 2) == 4 * 4 + tail
    assert f(5, 3) == 4 * 16 + tail
    assert f(257, 130) == 4 * 33412 + tail
    assert f(32768, 32768) == 4 * (1 << 30) + tail           # no 32-bit overflow
    assert f(1, 9) == 0 and f(9, 1) == 0 and f(0, 0) == 0
    assert _capi.lib().hf_grid_blocks(1 << 40, 0) == 16384    # the partial rows cover every grid of that family


def _call(lib, fn, W=17, H=9, lam=19.0, warm=0, max_iter=8, tol=1e-6, null=(), alias=False, misalign=False):
    _, arg = stand_ins(null)
    if fn == "hf_large_steps_apply":
        return lib.hf_large_steps_apply(W, H, lam, arg("v"), arg("v") if alias else arg("u", 4096), None)
    return lib.hf_large_steps_solve(W, H, lam, arg("u"), arg("u") if alias else arg("v", 4096), warm, max_iter, tol,
                                    arg("workspace", 8192 + (4 if misalign else 0)), arg("info", 64), None)


GRID = [{"W": 1}, {"H": 1}, {"W": 0}, {"H": 0}, {"W": 32770}, {"H": 32770}, {"W": 32769, "H": 32769},
        {"lam": -1e-3}, {"lam": NAN}, {"lam": INF}, {"lam": -INF}, {"alias": True}]
CASES = {
    "hf_large_steps_apply": GRID + [{"null": ("v",)}, {"null": ("u",)}],
    "hf_large_steps_solve": GRID + [{"null": ("u",)}, {"null": ("v",)}, {"null": ("workspace",)}, {"tol": -1e-9}, {"tol": NAN},
                                    {"max_iter": 0}, {"misalign": True}, {"warm": 1, "max_iter": 0}],
}


@pytest.mark.parametrize("fn", sorted(CASES))
def test_bad_arguments_are_refused(fn):
    assert_refused(_call, fn, CASES[fn])


def test_python_argument_checks():
    import torch
    import hf_amd
    for kw in ({"width": 1, "height": 8}, {"width": 8, "height": 1}, {"width": 8, "height": 8, "lambda_": -1.0},
               {"width": 8, "height": 8, "lambda_": NAN}, {"width": 8, "height": 8, "max_iter": 0},
               {"width": 8, "height": 8, "tol": -1e-3}, {"width": 8, "height": 8, "tol": NAN}):
        with pytest.raises(ValueError):
            hf_amd.LargeSteps(**kw)
    ls = hf_amd.LargeSteps(8, 6)
    assert (ls.width, ls.height, ls.lambda_, ls.max_iter, ls.tol) == (8, 6, 19.0, 256, 1e-6)
    with pytest.raises(ValueError):
        ls.to_differential(torch.zeros(6, 8))          # a host tensor: there is no CPU path
    with pytest.raises(ValueError):
        ls.from_differential(torch.zeros(6, 8))
    with pytest.raises(RuntimeError):
        ls.last_info()
