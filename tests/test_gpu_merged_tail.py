"""The merged tail (k_wf_merge): from round R on, every K neighbouring tasks of a batch run their remaining rounds as ONE
task of k_wf_tail.  Where a path's record lies shows nowhere in the result, so every (R, K) gives the film and the counters of the
default schedule, bit for bit; what changes is how many k_wf_ext launches there are (rounds 0..R: R + 1) and what they test.

All teapot cases use the 64 x 48, 10 spp tile of test_gpu_parity.py's test_wavefront_sample_chunking_and_paths_agree; with
HRT_WF_TASK_SIZE=64 it has 480 tasks.  Factor 7 does not divide 480 (the last merged task is short, and its top lies in the slack
beyond the slots), factor 480 puts every path into one task; rounds 0 and 1 have every task full or nearly full (destination == source,
and overlapping copies)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H, SPP = 64, 48, 10
ROUNDS = (0, 1, 2, 7, 49)
FACTORS = (2, 7, 480)
KNOBS = ("HRT_WF_MERGE_ROUND", "HRT_WF_MERGE_FACTOR", "HRT_WF_TASK_SIZE", "HRT_WF_TAIL_ROUND", "HRT_WF_MAX_SLOTS", "HRT_WF_DYNAMIC_TASKS")


def _bits(a):
    return a.view(np.uint32)


def _counters(st):
    return (st.rays, st.samples, st.box_tests, st.tri_tests)


@pytest.fixture(scope="module")
def tile(built, assets, scenes_dir):
    """The scene, and once for all tests: the default render, the megakernel's, and per R the un-merged run with HRT_WF_TAIL_ROUND=R+1
    (rounds 0..R launch by launch, as the merged run's) at task size 64."""
    import os
    from hobbyraytracer_amd import api
    saved = {k: os.environ.pop(k, None) for k in KNOBS}
    hs = api.HostScene(f"{scenes_dir}/teapot_scene.yaml", assets)
    dev = api.DeviceScene(hs.flat_ptr, 0)
    cam = hs.camera(W, H)
    p = api.default_params(W, H, SPP, stats=True, timing=True)
    one, s1 = dev.render_tile(cam, p)
    mega, s2 = dev.render_tile(cam, api.default_params(W, H, SPP, stats=True, megakernel=True))
    assert np.array_equal(_bits(one), _bits(mega)) and _counters(s1) == _counters(s2)
    unmerged = {}
    os.environ["HRT_WF_TASK_SIZE"] = "64"
    for r in ROUNDS:
        os.environ["HRT_WF_TAIL_ROUND"] = str(r + 1)
        img, st = dev.render_tile(cam, p)
        assert np.array_equal(_bits(one), _bits(img)) and st.traversal_launches == r + 1
        unmerged[r] = st
    del os.environ["HRT_WF_TASK_SIZE"], os.environ["HRT_WF_TAIL_ROUND"]
    yield dev, cam, p, one, s1, unmerged
    dev.close()
    for k, v in saved.items():
        if v is not None:
            os.environ[k] = v


@pytest.mark.parametrize("factor", FACTORS)
@pytest.mark.parametrize("r", ROUNDS)
def test_any_merge_round_and_factor_gives_the_default_film_and_counters(tile, monkeypatch, r, factor):
    dev, cam, p, one, s1, unmerged = tile
    monkeypatch.setenv("HRT_WF_TASK_SIZE", "64")
    monkeypatch.setenv("HRT_WF_MERGE_ROUND", str(r))
    monkeypatch.setenv("HRT_WF_MERGE_FACTOR", str(factor))
    img, st = dev.render_tile(cam, p)
    assert np.array_equal(_bits(one), _bits(img))
    assert _counters(st) == _counters(s1)
    # the merge really happened: rounds 0..R ran their k_wf_ext launches, and those tested what the same launches of the un-merged
    # schedule test
    u = unmerged[r]
    assert st.traversal_launches == r + 1
    assert (st.traversal_box_tests, st.traversal_tri_tests) == (u.traversal_box_tests, u.traversal_tri_tests)


@pytest.mark.parametrize("r,factor", [(0, 7), (2, 2), (7, 480)])
def test_merged_tasks_pulled_dynamically(tile, monkeypatch, r, factor):
    """HRT_WF_DYNAMIC_TASKS=1: the tail's waves pull the merged tasks from the group counters instead of taking the task of their number."""
    dev, cam, p, one, s1, unmerged = tile
    monkeypatch.setenv("HRT_WF_TASK_SIZE", "64")
    monkeypatch.setenv("HRT_WF_DYNAMIC_TASKS", "1")
    monkeypatch.setenv("HRT_WF_MERGE_ROUND", str(r))
    monkeypatch.setenv("HRT_WF_MERGE_FACTOR", str(factor))
    img, st = dev.render_tile(cam, p)
    assert np.array_equal(_bits(one), _bits(img))
    assert _counters(st) == _counters(s1) and st.traversal_launches == r + 1


@pytest.mark.parametrize("r,factor", [(1, 7), (7, 2)])
def test_every_batch_is_merged(tile, monkeypatch, r, factor):
    """HRT_WF_MAX_SLOTS = W H 3: four batches of 3 + 3 + 3 + 1 samples (144 tasks, and 48 in the last), each merged."""
    dev, cam, p, one, s1, unmerged = tile
    monkeypatch.setenv("HRT_WF_TASK_SIZE", "64")
    monkeypatch.setenv("HRT_WF_MAX_SLOTS", str(W * H * 3))
    monkeypatch.setenv("HRT_WF_MERGE_ROUND", str(r))
    monkeypatch.setenv("HRT_WF_MERGE_FACTOR", str(factor))
    img, st = dev.render_tile(cam, p)
    assert np.array_equal(_bits(one), _bits(img))
    assert _counters(st) == _counters(s1) and st.traversal_launches == 4 * (r + 1)


def _render(dev, cam, monkeypatch, env, **flags):
    from hobbyraytracer_amd import api
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    return dev.render_tile(cam, api.default_params(48, 48, 4, stats=True, timing=True, **flags))


def test_scene_without_a_mesh_merges(built, tmp_path, monkeypatch):
    """No traversal at all: the merge follows round R - 1's shading directly."""
    from hobbyraytracer_amd import api
    from tests.scene_helpers import random_world, films_equal
    hs = api.HostScene(random_world(tmp_path, 3, False), str(tmp_path))
    dev = api.DeviceScene(hs.flat_ptr, 0)
    cam = hs.camera(48, 48)
    one, s1 = _render(dev, cam, monkeypatch, {})
    mega, s2 = _render(dev, cam, monkeypatch, {}, megakernel=True)
    assert films_equal(one, mega) and s1.rays == s2.rays
    for r, factor in ((0, 2), (3, 5), (49, 36)):
        img, st = _render(dev, cam, monkeypatch, {"HRT_WF_TASK_SIZE": "64", "HRT_WF_MERGE_ROUND": str(r), "HRT_WF_MERGE_FACTOR": str(factor)})
        assert films_equal(one, img), (r, factor)
        assert _counters(st) == _counters(s1) and st.traversal_launches == 0, (r, factor)
    dev.close()


def test_scene_with_two_meshes_ignores_the_knob(built, tmp_path, monkeypatch):
    """With several meshes k_wf_tail would prepare round R's further meshes a second time: such a scene keeps its schedule whatever the
    knob says.  Its schedule: this tile is a tiny batch, which by default runs round 0's two k_wf_ext launches and then the tail; told to
    run every round launch by launch (HRT_WF_TAIL_ROUND=50) it has 50 x 2 of them, with the knob as without."""
    from hobbyraytracer_amd import api
    from tests.scene_helpers import many_meshes_scene, films_equal
    hs = api.HostScene(many_meshes_scene(tmp_path, 2), str(tmp_path))
    dev = api.DeviceScene(hs.flat_ptr, 0)
    cam = hs.camera(48, 48)
    knob = {"HRT_WF_TASK_SIZE": "64", "HRT_WF_MERGE_ROUND": "5", "HRT_WF_MERGE_FACTOR": "4"}
    one, s1 = _render(dev, cam, monkeypatch, {"HRT_WF_TASK_SIZE": "64"})
    img, st = _render(dev, cam, monkeypatch, knob)
    assert films_equal(one, img)
    assert _counters(st) == _counters(s1)
    assert st.traversal_launches == s1.traversal_launches == 2
    assert (st.traversal_box_tests, st.traversal_tri_tests) == (s1.traversal_box_tests, s1.traversal_tri_tests)
    one50, s50 = _render(dev, cam, monkeypatch, {"HRT_WF_TASK_SIZE": "64", "HRT_WF_TAIL_ROUND": "50"})
    img50, st50 = _render(dev, cam, monkeypatch, dict(knob, HRT_WF_TAIL_ROUND="50"))
    assert films_equal(one, one50) and films_equal(one, img50)
    assert st50.traversal_launches == s50.traversal_launches == 50 * 2
    dev.close()


def test_next_event_estimation_ignores_the_knob(tile, monkeypatch):
    """k_wf_tail has no stage for the shadow rays: HRT_FLAG_NEE renders round by round, all 50 of them."""
    from hobbyraytracer_amd import api
    dev, cam, p, one, s1, unmerged = tile
    pn = api.default_params(W, H, SPP, stats=True, timing=True, nee=True)
    monkeypatch.setenv("HRT_WF_TASK_SIZE", "64")
    ref, sr = dev.render_tile(cam, pn)
    assert sr.shadow_rays > 0, "the scene must have a table light"
    monkeypatch.setenv("HRT_WF_MERGE_ROUND", "2")
    monkeypatch.setenv("HRT_WF_MERGE_FACTOR", "7")
    img, st = dev.render_tile(cam, pn)
    assert np.array_equal(_bits(ref), _bits(img))
    assert _counters(st) == _counters(sr) and st.shadow_rays == sr.shadow_rays
    assert st.traversal_launches == sr.traversal_launches == 50


@pytest.mark.parametrize("enclosed", [True, False])
def test_stale_front_face_scene_ignores_the_knob(built, tmp_path, monkeypatch, enclosed):
    """... nor for the stale frontFace (k_wf_stale); the scene has three meshes besides."""
    from hobbyraytracer_amd import api
    from tests.scene_helpers import stale_front_face_scene, films_equal
    hs = api.HostScene(stale_front_face_scene(tmp_path, enclosed), str(tmp_path))
    dev = api.DeviceScene(hs.flat_ptr, 0)
    cam = hs.camera(48, 48)
    one, s1 = _render(dev, cam, monkeypatch, {"HRT_WF_TASK_SIZE": "64"})
    img, st = _render(dev, cam, monkeypatch, {"HRT_WF_TASK_SIZE": "64", "HRT_WF_MERGE_ROUND": "2", "HRT_WF_MERGE_FACTOR": "4"})
    assert films_equal(one, img)
    assert _counters(st) == _counters(s1) and st.traversal_launches == s1.traversal_launches == 50 * 3
    dev.close()
