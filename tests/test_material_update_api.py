"""Material and emission edits without a GPU: the two new symbols of the C ABI and their Python wrappers, the argument checks
that fire on the host before any HIP call (a NULL scene), and pt_debug_packed's new array in the header next to the old ones."""
import os

import numpy as np

NEW_SYMBOLS = ("pt_scene_update_materials", "pt_scene_update_emission")


def _err(api):
    return api.lib().pt_last_error().decode()


def test_new_symbols_are_declared_and_exported(api):
    from conftest import ROOT
    L = api.lib()
    header = open(os.path.join(ROOT, "include", "pt_api.h")).read()
    for n in NEW_SYMBOLS:
        assert hasattr(L, n), n
        assert n + "(" in header, n


def test_wrappers_exist(api):
    assert all(hasattr(api.Scene, n) for n in ("update_materials", "update_emission", "packed", "generation", "has_motion"))
    assert "update_materials" in api.Scene.generation.__doc__ and "update_emission" in api.Scene.generation.__doc__
    assert "mats" in api.Scene.packed.__doc__


def test_null_scene_is_refused_with_a_message(api):
    L = api.lib()
    mats = np.zeros(2 * 176, np.uint8)
    idx = np.zeros(1, np.int32)
    em = np.ones((1, 4), np.float32)
    assert L.pt_scene_update_materials(None, mats.ctypes.data, 2) == -1 and "pt_scene_update_materials: null scene" in _err(api)
    assert L.pt_scene_update_materials(None, None, 0) == -1 and "pt_scene_update_materials: null scene" in _err(api)
    assert L.pt_scene_update_emission(None, 1, idx.ctypes.data, em.ctypes.data) == -1 and "pt_scene_update_emission: null scene" in _err(api)
    assert L.pt_scene_update_emission(None, 0, None, None) == -1 and "pt_scene_update_emission: null scene" in _err(api)


def test_debug_packed_lists_the_materials_and_the_old_arrays(api):
    from conftest import ROOT
    header = open(os.path.join(ROOT, "include", "pt_api.h")).read()
    assert "4 materials 96 B" in header                   # pt_debug_packed's new array
    for old in ("0 nodes 64 B", "1 triangles 48 B", "2 attributes 80 B", "3 lights 64 B"):
        assert old in header, old


def test_wrapper_refuses_a_ragged_material_array(api):
    """176 bytes per record, checked in Python before the call: no scene is needed to see it."""
    import pytest
    sc = api.Scene.__new__(api.Scene)
    sc.h = None
    with pytest.raises(api.PtError, match="176-byte"):
        sc.update_materials(np.zeros(177, np.uint8))
    with pytest.raises(api.PtError, match="float3 or float4"):
        sc.update_emission([0], np.zeros((1, 2), np.float32))
