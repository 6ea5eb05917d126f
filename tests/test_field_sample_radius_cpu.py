"""CPU: the interface of streamed field sampling for 'radius' / 'bidirectional' decoders is in place -- the per-query union entry points
(gaot_nbr_union_grid_count / gaot_nbr_union_grid_fill, csrc/graph.hip) are declared in the header, bound in _lib.SIGNATURES with the
header's argument counts and exported by the library, with the ABI still version 11; graph.query_lists exists and refuses, on the
host, what it does not handle."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"gaot_nbr_union_grid_count": 9, "gaot_nbr_union_grid_fill": 11}


def test_union_symbols_declared_bound_and_exported():
    from gaot_3d_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gaot3d_hip.h")).read(), flags=re.S)
    lib = _lib.load()
    for name, nargs in NAMES.items():
        m = re.search(r"\b" + name + r"\s*\(([^)]*)\)", src)
        assert m, f"{name} is not declared in include/gaot3d_hip.h"
        assert name in _lib.SIGNATURES, f"{name} is not in _lib.SIGNATURES"
        assert len(m.group(1).split(",")) == len(_lib.SIGNATURES[name][1]) == nargs, \
            f"{name}: header and SIGNATURES disagree on the arguments"
        assert hasattr(lib, name), f"{name} is not exported by libgaot3d_hip.so"
    assert lib.gaot_abi_version() == 11


def test_query_lists_exists_and_checks_on_the_host():
    from gaot_3d_amd import graph
    from gaot_3d_amd._lib import GaotError
    assert callable(graph.query_lists)
    grid = graph.LatentGrid((2, 2, 2), (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0), torch.zeros(8, 3))
    with pytest.raises(ValueError, match="strategy"):
        graph.query_lists("knn", torch.zeros(4, 3), grid, 0.5, 1)
    with pytest.raises(GaotError, match="HIP device only"):
        graph.query_lists("bidirectional", torch.zeros(4, 3), grid, 0.5, 1)
