"""CPU: the fp32 restatement of process_mask_native (tests/mask_native_ref.py) against the reference's own function, recorded in
tests/golden/mask_native.npz by scripts/make_golden_mask_native.py -- bit for bit, for every case and both prototype dtypes.  The kernel
tests accept results against this restatement, so it is pinned first."""
import numpy as np
import pytest

from tests import mask_native_ref as mr


@pytest.mark.parametrize("pd", mr.PROTO_DTYPES)
@pytest.mark.parametrize("name", list(mr.CASES))
def test_restatement_equals_reference_golden(name, pd):
    bits, v64, band = mr.reference(name, pd)
    g = mr.golden(name, pd)
    c, mh, mw, h0, w0, wr, wc = mr.CASES[name]
    assert g.shape == (mr.N, h0, w0) and bits.shape == g.shape
    assert np.array_equal(bits, g)
    top, left, bottom, right = mr.window(mh, mw, (h0, w0))
    assert (bottom - top, right - left) == (wr, wc)
    assert g[0].any() and not g[1].any()     # the whole-image box has pixels, the empty box has none
    # the fp64 evaluation agrees with the fp32 one except within the band of 0.5 (on these inputs: everywhere)
    d = bits != (v64 > 0.5)
    assert 0 < band < 1e-4
    assert not d.any() or np.abs(v64[d] - 0.5).max() <= band


def test_window_matches_the_product_side():
    from yolov5_amd.segment import native_window

    for c, mh, mw, h0, w0, _, _ in mr.CASES.values():
        assert native_window(mh, mw, (h0, w0)) == mr.window(mh, mw, (h0, w0))
    for shape in ((1080, 810), (720, 1280), (1, 1), (3, 1000)):
        assert native_window(160, 160, shape) == mr.window(160, 160, shape)
    with pytest.raises(ValueError, match="empty window"):
        native_window(25, 40, (1, 300))      # the content is 0.13 of a row in the middle of row 12: both int() give 12 (torch raises there)
    with pytest.raises(ValueError):
        native_window(24, 40, (0, 10))
