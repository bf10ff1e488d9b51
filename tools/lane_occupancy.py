#!/usr/bin/env python3
"""Lane occupancy of the logic step and rays traced by the TIMED kernel, from a -DPT_STAMPS diagnostic build (PT_LIB_PATH).

usage: PT_LIB_PATH=.../lib_stamps.so python tools/lane_occupancy.py [spp] [scene] [name=value ...]
A lane serves one pixel of its wave's tile; once that pixel has had its samples the lane idles through every further logic
step of the wave. busy_share = lanes that shade a hit or start a sample / (64 x logic steps of waves), over one 1920x1080 frame.
The counting pass of the same frame gives the reference's ray counts; the timed kernel traces fewer shadow rays (pt_path.h).
Never quote this build's run time.
"""
import json, os, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from cudapathtracer_amd import api, scenes
spp = int(sys.argv[1]) if len(sys.argv) > 1 else 64
wl = sys.argv[2] if len(sys.argv) > 2 else "cornell"
opts = api.parse_options([a for a in sys.argv[3:] if "=" in a])
tmp = tempfile.mkdtemp()
s = getattr(scenes, wl)(tmp, width=1920, height=1080, spp=spp, max_depth=8)
hs = api.HostScene(s["config"]); sc = api.Scene(hs, options=opts)
tiles = torch.zeros(api.n_tiles(1920, 1080), 64, 4, device="cuda")
sc.reset_counters()
sc.render_tiles_device(hs.camera(), 1920, 1080, spp, 8, tiles.data_ptr(), count_work=False)
torch.cuda.synchronize()
flags = sc.flags()
c, st = sc.counters(), sc.debug_stamps()
sc.reset_counters()
tiles.zero_()
sc.render_tiles_device(hs.camera(), 1920, 1080, spp, 8, tiles.data_ptr(), count_work=True)
torch.cuda.synchronize()
ref = sc.counters()
slots, busy = st["slot7"], c["iterations"]
out = {"scene": wl, "spp": spp, "options": opts, "kernel_flags": flags, "lane_slots": slots, "busy_lanes": busy,
       "busy_share": busy / slots if slots else None, "idle_share": 1.0 - busy / slots if slots else None,
       "timed_rays_closest": c["rays_closest"], "timed_rays_shadow": c["rays_shadow"],
       "reference_rays_closest": ref["rays_closest"], "reference_rays_shadow": ref["rays_shadow"],
       "shadow_rays_dropped_share": 1.0 - c["rays_shadow"] / ref["rays_shadow"] if ref["rays_shadow"] else None}
print(json.dumps(out))
