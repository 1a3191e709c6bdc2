"""The library and the host harness classify a scene with one function (mtr_scene_host.cpp classify_scene): for every pinned
scene mtr_scene_traits reports the harness's word — a copy into the device scene that forgets a field shows here — and
MTR_MODE_AUTO resolves to the organisation recorded with it."""
import pytest

import scene_class_cases as cases
from scene_class_cases import host_class, planned_mode
from test_scene_class import EXPECTED

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(EXPECTED))
def test_library_reports_the_harness_word(host_harness, tmp_path, name):
    scene = cases.CASES[name](tmp_path)
    assert scene.gpu_traits() == host_class(host_harness, scene)[0] == EXPECTED[name][0]
    assert planned_mode(scene) == EXPECTED[name][3]


def test_recolouring_a_scene_on_the_device_reclassifies_it(host_harness, tmp_path):
    """params.update() on a scene that is on the device (mtr_scene_set_colors): kTrGrey follows the new tables, both ways"""
    scene = cases.grey_cornell(tmp_path)
    assert scene.gpu_traits() == EXPECTED["grey-cornell"][0]
    cases.recolour(scene, (0.6, 0.2, 0.1))
    assert scene.gpu_traits() == host_class(host_harness, scene)[0] == EXPECTED["grey-cornell-one-wall-coloured"][0]
    cases.recolour(scene, (0.4, 0.4, 0.4))
    assert scene.gpu_traits() == EXPECTED["grey-cornell"][0]
