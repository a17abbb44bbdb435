"""The render-mode compositing entries (depth channel, backgrounds) check their arguments before any HIP call: no GPU
needed."""
import pytest


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from edgegaussians_amd import _lib
    return _lib


def _fwd(h, C=1, N=4, colors=None, cpc=0, channels=3, depth=1, bg=None, offsets=1, flat=1, w=32, hh=32, render=1,
         alphas=1, last=1):
    return h.eg_composite_fwd_modes_cams(C, 1, N, colors, cpc, channels, depth, bg, offsets, flat, w, hh, render, alphas,
                                         last, None)


def _bwd(h, C=1, N=4, colors=None, cpc=0, channels=3, depth=1, bg=None, v_colors=None, v_depths=1):
    return h.eg_composite_bwd_modes_cams(C, 1, N, colors, cpc, channels, depth, bg, 1, 1, 32, 32, 1, 1, 1, None, 1,
                                         v_colors, v_depths, None)


@pytest.mark.parametrize("case", ["channels", "no_channels_no_depth", "neither_depth_nor_bg", "null", "null_colors",
                                  "sizes"])
def test_forward_rejects_bad_arguments(lib, case):
    h = lib.load(require_device=False)
    kw = {"channels": dict(channels=2, colors=1), "no_channels_no_depth": dict(channels=0, depth=0, bg=1),
          "neither_depth_nor_bg": dict(colors=1, depth=0), "null": dict(colors=1, render=None),
          "null_colors": dict(channels=3), "sizes": dict(colors=1, C=0)}[case]
    assert _fwd(h, **kw) == -1
    assert b"eg_composite_fwd_modes_cams" in h.eg_last_error_string()


@pytest.mark.parametrize("case", ["channels", "no_channels_no_depth", "neither_depth_nor_bg", "null_colors",
                                  "null_v_depths", "sizes"])
def test_backward_rejects_bad_arguments(lib, case):
    h = lib.load(require_device=False)
    kw = {"channels": dict(channels=4, colors=1), "no_channels_no_depth": dict(channels=0, depth=0, bg=1),
          "neither_depth_nor_bg": dict(colors=1, depth=0), "null_colors": dict(channels=1),
          "null_v_depths": dict(colors=1, v_depths=None), "sizes": dict(colors=1, N=-1)}[case]
    assert _bwd(h, **kw) == -1
    assert b"eg_composite_bwd_modes_cams" in h.eg_last_error_string()

