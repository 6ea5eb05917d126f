"""CPU: the fused PointNet GeometricEmbedding entry points (csrc/pointnet.hip) are part of the C ABI -- declared in the header,
bound in _lib.SIGNATURES with the header's argument counts, exported by the library -- and the ABI stays version 11."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("gaot_pointnet_fwd", "gaot_pointnet_bwd", "gaot_pointnet_bwd_parts")


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gaot3d_hip.h")).read(), flags=re.S)


def test_pointnet_symbols_declared_bound_and_exported():
    from gaot_3d_amd import _lib
    src = _header()
    lib = _lib.load()
    for name in NAMES:
        m = re.search(r"\b" + name + r"\s*\(([^)]*)\)", src)
        assert m, f"{name} is not declared in include/gaot3d_hip.h"
        assert name in _lib.SIGNATURES, f"{name} is not in _lib.SIGNATURES"
        assert len(m.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), f"{name}: header and SIGNATURES disagree on the arguments"
        assert hasattr(lib, name), f"{name} is not exported by libgaot3d_hip.so"
    assert lib.gaot_abi_version() == 11


def test_pointnet_bwd_parts_is_bounded():
    """the partial table's row count does not grow with E (grid-stride workgroups), and is at least one row"""
    from gaot_3d_amd import _lib
    lib = _lib.load()
    parts = [int(lib.gaot_pointnet_bwd_parts(e)) for e in (0, 1, 255, 256, 257, 5000, 4_000_000, 2_000_000_000)]
    assert parts[0] == 1 and parts[1] == 1 and parts[3] == 1 and parts[4] == 2 and parts[5] == 20
    assert 256 < parts[-2] <= 512 and 256 < parts[-1] <= 512      # PN_BWD_PARTS = 512: the most rows, whatever E is
    # every workgroup has a span of its own: 513 tiles of 256 edges are 2 tiles each for 257 workgroups, not 512 half of them idle
    assert int(lib.gaot_pointnet_bwd_parts(513 * 256)) == 257
    assert all(1 <= int(lib.gaot_pointnet_bwd_parts(t * 256)) <= 512 for t in range(1, 2100, 7))
