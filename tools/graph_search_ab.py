#!/usr/bin/env python3
"""A/B of the grid neighbour searches (gaot_knn_grid, gaot_radius_grid_count, gaot_nbr_union_grid_count) between builds of the library:

    python tools/graph_search_ab.py parent=/path/to/other/libgaot3d_hip.so [name=path ...]

The in-tree build is always measured as `tree`.  4 M random queries against the 64 x 64 x 32 token grid; the builds alternate in one
process, device events around each call, median (min, max) of 7 rounds, and the outputs of all builds are compared (`identical`).  A
build that lacks an entry point is left out of that entry point's rows."""
import ctypes as C
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gaot_3d_amd import graph  # noqa: E402
from gaot_3d_amd.data import latent_grid  # noqa: E402

p_, i_, i64_, f_ = C.c_void_p, C.c_int, C.c_int64, C.c_float
SIGS = {"gaot_knn_grid": [p_, i64_, p_, p_, i_, p_, p_], "gaot_radius_grid_count": [p_, i64_, p_, p_, f_, i_, p_, p_],
        "gaot_nbr_union_grid_count": [p_, i64_, p_, p_, i_, f_, i_, p_, p_]}
libs = {"tree": C.CDLL(os.path.join(ROOT, "gaot_3d_amd", "lib", "libgaot3d_hip.so"))}
for a in sys.argv[1:]:
    name, path = a.split("=", 1)
    libs[name] = C.CDLL(path)
for lib in libs.values():
    for fn, args in SIGS.items():
        if hasattr(lib, fn):
            getattr(lib, fn).restype, getattr(lib, fn).argtypes = i_, args

dev, latent, n, reps = "cuda:0", (64, 64, 32), 4000000, 7
grid = graph.as_latent_grid(latent_grid(latent).to(dev), latent)
gs = grid.c_struct()
torch.manual_seed(0)
q = (torch.rand(n, 3, device=dev) * 2 - 1).contiguous()
ptr = lambda t: C.c_void_p(t.data_ptr())
st = C.c_void_p(torch.cuda.current_stream().cuda_stream)


def row(title, fn, call, shape):
    have = {a: l for a, l in libs.items() if hasattr(l, fn)}
    outs = {a: torch.empty(*shape, dtype=torch.int32, device=dev) for a in have}
    for a, l in have.items():
        assert call(getattr(l, fn), outs[a]) == 0
    torch.cuda.synchronize()
    ts = {a: [] for a in have}
    for _ in range(reps):
        for a, l in have.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); call(getattr(l, fn), outs[a]); e1.record()
            torch.cuda.synchronize()
            ts[a].append(e0.elapsed_time(e1))
    first = next(iter(outs.values()))
    same = all(torch.equal(first, o) for o in outs.values())
    print(f"{title} n={n}: " + ", ".join(f"{a} {sorted(v)[reps // 2]:.3f} ms ({min(v):.3f}, {max(v):.3f})" for a, v in ts.items())
          + f"; identical: {same}", flush=True)


for k in (1, 4, 8, 12, 16, 24, 32, 48, 64):
    row(f"gaot_knn_grid k={k:2d}", "gaot_knn_grid", lambda f, o: f(ptr(q), n, C.byref(gs), ptr(grid.pos), k, ptr(o), st), (n, k))
for r in (0.033, 0.1):
    row(f"gaot_radius_grid_count r={r}", "gaot_radius_grid_count",
        lambda f, o: f(ptr(q), n, C.byref(gs), ptr(grid.pos), r, 32, ptr(o), st), (n,))
for k in (1, 8, 32):
    row(f"gaot_nbr_union_grid_count k={k:2d} r=0.033", "gaot_nbr_union_grid_count",
        lambda f, o: f(ptr(q), n, C.byref(gs), ptr(grid.pos), k, 0.033, 32, ptr(o), st), (n,))
