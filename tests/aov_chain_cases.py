"""The scenes, cameras and sizes of the chain pass's oracle-parity cases (test_aov_chain.py), chosen on the CPU with
aov_chain_ref so that together they hold every class of ray: test_aov_chain_api.py checks that without a GPU."""
import os

from conftest import golden_scene

SEED = 103033

# name: (scene, w, h, camera or None for the scene's own, aov_spp, max_links)
#   camera: (pinhole, pos, rot, fov, aperture, focal_dist)
_GLASS_LENS = (False, (0.15, -0.1, 1.2), (3.0, -8.0, 2.0), 55.0, 0.08, 2.2)
CASES = {
    "mixed32_l1": ("mixed32", 32, 32, None, 1, 1),
    "mixed32_l2": ("mixed32", 32, 32, None, 1, 2),
    "mixed32_l8": ("mixed32", 32, 32, None, 1, 8),
    "glass_mirror_40x24": ("glass_mirror", 40, 24, _GLASS_LENS, 3, 8),
    "glass_mirror_13x9": ("glass_mirror", 13, 9, (False, (0.1, -0.2, 0.9), (-4.0, 6.0, 0.0), 62.0, 0.05, 2.0), 2, 4),
    "textured_mirror_wall": ("textured_mirror", 32, 32, (True, (-0.5, 0.1, 0.8), (-8.0, -28.0, 0.0), 60.0, 0.0, 0.0), 1, 4),
}


def scene_config(scene, scene_dir):
    from cudapathtracer_amd import scenes
    if scene == "mixed32":
        return golden_scene("mixed32")
    out = os.path.join(scene_dir, "chain_" + scene)
    if scene == "glass_mirror":       # glass tall box, mirror short box
        return scenes.cornell(out, width=40, height=24, spp=4, max_depth=8, tall_material=5, short_material=19, name="chain_gm")["config"]
    if scene == "textured_mirror":    # textured floor and back wall seen in a mirror right wall
        return scenes.textured(out, name="chain_tex", right_material=19)["config"]
    raise KeyError(scene)


def case(api, name, scene_dir):
    """(config path, camera, w, h, aov_spp, max_links) of a case."""
    scene, w, h, cam, aov_spp, max_links = CASES[name]
    cfg = scene_config(scene, scene_dir)
    if cam is None:
        camera = api.HostScene(cfg).camera()
    else:
        pinhole, pos, rot, fov, ap, fd = cam
        camera = api.make_camera(pinhole, pos, rot, fov, w, h, ap, fd)
    return cfg, camera, w, h, aov_spp, max_links
