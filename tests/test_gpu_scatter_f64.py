"""The depth-limited films of tests/f64_scatter_cases.py on the HIP kernels, on all three render paths (per-round wavefront
kernels, k_wf_tail, the megakernel): every film must pass the float64 check that tests/test_scatter_f64.py has already shown the
oracle to pass, and must equal the oracle's film of the same scene and parameters bit for bit."""
import numpy as np
import pytest

from tests import f64_cases as C
from tests import f64_scatter_cases as SC

pytestmark = pytest.mark.gpu

PATHS = ["wavefront-rounds", "wavefront-tail", "megakernel"]


def _params(case, path=None):
    from hobbyraytracer_amd import api
    return api.default_params(SC.W, SC.H, 1, seed=C.SEED, max_depth=SC.CASES[case]["max_depth"], megakernel=(path == "megakernel"))


def _device(hs, path, monkeypatch):
    from hobbyraytracer_amd import api
    monkeypatch.setenv("HRT_WF_TAIL_ROUND", "1000" if path == "wavefront-rounds" else "1")
    return api.DeviceScene(hs.flat_ptr, 0)


@pytest.fixture(scope="module")
def oracle_films(built, tmp_path_factory):
    """The oracle's film of every case, rendered once and shared by the three paths."""
    from oracle import oracle_py
    films = {}
    for case in SC.CASES:
        hs = SC.build_scene(tmp_path_factory.mktemp(case), case)
        films[case], _ = oracle_py.World(hs.flat_ptr).render_tile(hs.camera(SC.W, SC.H), _params(case))
        films[case].setflags(write=False)
    return films


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("case", sorted(SC.CASES))
def test_depth_limited_film(built, tmp_path, oracle_films, case, path, monkeypatch):
    hs = SC.build_scene(tmp_path, case)
    film, _ = _device(hs, path, monkeypatch).render_tile(hs.camera(SC.W, SC.H), _params(case, path))
    print(f"{case} {path}: ambiguous share {SC.check_film(film, case):.5f}")
    want = oracle_films[case]
    assert np.array_equal(film.view(np.uint32), want.view(np.uint32)), \
        f"{int((film.view(np.uint32) != want.view(np.uint32)).any(-1).sum())} pixels differ from the oracle's film"
