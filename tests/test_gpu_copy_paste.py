"""GPU (-m gpu): the copy-paste augmentation on the MI355X -- the twins of tests/test_emu_copy_paste.py through the library on the device
(reference-generated goldens, bit-identical; y5_paste_planes and y5_mosaic_batch_paste against the restatement; the no-plane identity; the
geometry check that does not rest on the restatement) and one raster case at the production canvas (S2 = 1280: 40 row bands, a handful of
polygons up to tile size on several planes) against `reference_planes`."""
import numpy as np
import pytest
import torch

from tests import copy_paste_ref as cp
from tests import test_emu_copy_paste as twin

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.mark.parametrize("kind,name,seed", twin.CASES)
def test_batches_match_reference_golden(kind, name, seed, dev):
    twin.check_golden(kind, name, seed, dev)


@pytest.mark.parametrize("name", [c[0] for c in twin.raster_cases()])
def test_paste_planes_match_restatement(name, dev):
    twin.check_raster(name, dev)


def test_paste_render_matches_restatement(dev):
    twin.check_render(dev)


def test_no_plane_launch_is_mosaic_batch(dev):
    twin.check_no_plane_identity(dev)


def test_fill_geometry_independent_of_the_restatement(dev):
    twin.check_geometry(dev)


def test_production_canvas_planes_match_restatement(dev):
    """S2 = 1280 (s = 640): the row pitch of 40 words (41 in LDS), 40 bands.  Polygons up to tile size (640), one touching all four canvas
    borders' coordinates 0 and 1280, a thin one inside a single band, overlapping ones, three planes with an empty one between."""
    S2 = 1280
    rng = np.random.default_rng(3)

    def blob(k, cx, cy, r):
        a = np.sort(rng.uniform(0, 2 * np.pi, k))
        rr = r * rng.uniform(0.4, 1.0, k)
        return np.clip(np.stack((cx + rr * np.cos(a), cy + rr * np.sin(a)), 1), 0, S2).astype(np.int32)

    items = [(blob(60, 320, 320, 320), 0), (blob(9, 900, 300, 250), 0), (blob(25, 500, 450, 200), 0),      # overlapping, up to tile size
             (np.array([[0, 0], [S2, 600], [640, S2], [0, 900]], np.int32), 2),                           # coordinates at 0 and at S2
             (np.array([[100, 1000], [1200, 1003], [600, 1010]], np.int32), 2), (blob(120, 1000, 1000, 400), 2)]
    polys, plane = [p for p, _ in items], [k for _, k in items]
    got = twin.kernel_planes(polys, plane, 3, S2, dev)
    ref = cp.reference_planes(polys, plane, 3, S2)
    assert got.shape == (3, S2, 40) and ref[0].any() and ref[2].any() and not got[1].any()
    assert np.array_equal(got, ref)
    assert np.array_equal(got, twin.kernel_planes(polys, plane, 3, S2, dev))      # no atomics on memory: run to run identical
