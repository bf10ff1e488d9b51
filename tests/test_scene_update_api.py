"""Dynamic geometry without a GPU: the five new symbols of the C ABI and their Python wrappers, and the argument checks of
pt_scene_update_mesh / pt_scene_update_vertices[_device] / pt_scene_generation / pt_preview_scene_changed that fire on the host
before any HIP call (a NULL scene, NULL arrays)."""
import ctypes
import os

import numpy as np

NEW_SYMBOLS = ("pt_scene_update_mesh", "pt_scene_update_vertices", "pt_scene_update_vertices_device", "pt_scene_generation",
               "pt_preview_scene_changed")


def _err(api):
    return api.lib().pt_last_error().decode()


def test_new_symbols_are_declared_and_exported(api):
    from conftest import ROOT
    L = api.lib()
    header = open(os.path.join(ROOT, "include", "pt_api.h")).read()
    for n in NEW_SYMBOLS:
        assert hasattr(L, n), n
        assert n + "(" in header, n
    assert all(hasattr(api.Scene, n) for n in ("update_mesh", "update_vertices", "generation"))
    assert hasattr(api.Preview, "scene_changed")
    assert "3 lights 64 B" in header                      # pt_debug_packed's new array


def test_null_scene_is_refused_with_a_message(api):
    L = api.lib()
    pts = np.zeros((4, 4), np.float32)
    d = api.SceneDesc()
    st = np.zeros(1, api.BUILD_STATS)
    p = pts.ctypes.data
    assert L.pt_scene_update_mesh(None, ctypes.byref(d), 2, st.ctypes.data) == -1 and "pt_scene_update_mesh: null scene" in _err(api)
    for fn in ("pt_scene_update_vertices", "pt_scene_update_vertices_device"):
        assert getattr(L, fn)(None, p, 4, p, 4, st.ctypes.data) == -1
        assert fn + ": null scene" in _err(api)
        assert getattr(L, fn)(None, None, 4, None, 0, None) == -1
        assert "null scene" in _err(api)
    assert L.pt_scene_generation(None) == -1 and "null scene" in _err(api)
    assert L.pt_preview_scene_changed(None, 0) == -1 and "null session" in _err(api)
    assert L.pt_preview_scene_changed(None, 1) == -1 and "null session" in _err(api)


def test_wrapper_refuses_arrays_without_a_leaf_size(api):
    """Only a HostScene knows its config's leaf size; a dict of arrays or a SceneDesc must bring one (checked in Python)."""
    import pytest
    with pytest.raises(api.PtError, match="max_leaf_size"):
        api.Scene._mesh_desc({"points": np.zeros(16, np.uint8)}, None)
    with pytest.raises(api.PtError, match="max_leaf_size"):
        api.Scene._mesh_desc(api.SceneDesc(), None)
