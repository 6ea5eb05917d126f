"""The launches of the two second-order field adjoints, pinned as tests/test_field_adjoint_launch_profile_gpu.py pins the three older
calls, on that file's decoders: a 'knn' decoder (k = 8) and a 'bidirectional' one (k = 1, r = 0.9), two scales with softmax weights,
C = 32, 70 queries on a 4 x 4 x 4 token grid in chunks of 32 (three chunks, the last one partial; four queries far outside the box).
MAGNODecoder.sample_directional_vjp runs with one and with three directions per query, with all three cotangents and with cot_d2
alone; sample_hessian_vjp with all three and with cot_hess alone.  Pinned: the number of library launches (ops.launch_count) and the
{timing label: calls} map (ops.timing_summary) of one call -- per chunk one jet forward and one jet adjoint per scale list (one list on
'knn', two on 'bidirectional') and one projection middle.  The calls of the older file, run beside these, still launch what it pins.

How the literals in EXPECTED were obtained: `_profile` below, as it stands, was run on an MI355X against the implementation this file
arrived with, and what it returned was pasted here; a change that moves them has changed what the API launches."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_field_adjoint_launch_profile_gpu as base  # noqa: E402  (_decoder, NQ, CHUNK, STRATEGIES)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
METHODS = ("directional_nd1", "directional_nd1_d2only", "directional_nd3", "directional_nd3_d2only", "hessian", "hessian_hessonly")

# (strategy, method) -> (library launches, {timing label: calls})
EXPECTED = {
    ('knn', 'directional_nd1'): (81, {'gno_adj_jet2_qd_nh2': 3, 'gno_jet2_knn_qd_nh2_d1': 3, 'mlp2_jet2_cot_mid_h256_d1': 3}),
    ('knn', 'directional_nd1_d2only'): (81, {'gno_adj_jet2_qd_nh2': 3, 'gno_jet2_knn_qd_nh2_d1': 3, 'mlp2_jet2_cot_mid_h256_d1': 3}),
    ('knn', 'directional_nd3'): (105, {'gno_adj_jet2_qd_nh2': 3, 'gno_jet2_knn_qd_nh2_d3': 3, 'mlp2_jet2_cot_mid_h256_d3': 3}),
    ('knn', 'directional_nd3_d2only'): (105, {'gno_adj_jet2_qd_nh2': 3, 'gno_jet2_knn_qd_nh2_d3': 3, 'mlp2_jet2_cot_mid_h256_d3': 3}),
    ('knn', 'hessian'): (141, {'gno_adj_jet2_nh2': 3, 'gno_jet2_knn_nh2_d6': 3, 'mlp2_jet2_cot_mid_h256_d6': 3}),
    ('knn', 'hessian_hessonly'): (141, {'gno_adj_jet2_nh2': 3, 'gno_jet2_knn_nh2_d6': 3, 'mlp2_jet2_cot_mid_h256_d6': 3}),
    ('bidirectional', 'directional_nd1'): (153, {'gno_adj_jet2_qd_nh2': 6, 'gno_jet2_rows_qd_nh2_d1': 6, 'mlp2_jet2_cot_mid_h256_d1': 3}),
    ('bidirectional', 'directional_nd1_d2only'): (153, {'gno_adj_jet2_qd_nh2': 6, 'gno_jet2_rows_qd_nh2_d1': 6, 'mlp2_jet2_cot_mid_h256_d1': 3}),
    ('bidirectional', 'directional_nd3'): (153, {'gno_adj_jet2_qd_nh2': 6, 'gno_jet2_rows_qd_nh2_d3': 6, 'mlp2_jet2_cot_mid_h256_d3': 3}),
    ('bidirectional', 'directional_nd3_d2only'): (153, {'gno_adj_jet2_qd_nh2': 6, 'gno_jet2_rows_qd_nh2_d3': 6, 'mlp2_jet2_cot_mid_h256_d3': 3}),
    ('bidirectional', 'hessian'): (153, {'gno_adj_jet2_nh2': 6, 'gno_jet2_rows_nh2_d6': 6, 'mlp2_jet2_cot_mid_h256_d6': 3}),
    ('bidirectional', 'hessian_hessonly'): (153, {'gno_adj_jet2_nh2': 6, 'gno_jet2_rows_nh2_d6': 6, 'mlp2_jet2_cot_mid_h256_d6': 3}),
}


def _profile(strategy, method):
    import gaot_3d_amd
    from gaot_3d_amd import ops
    gaot_3d_amd.set_precision("fp32")
    dec, rn, q, tokens, (gy, gj, gl) = base._decoder(strategy, 32, True)
    gen = torch.Generator().manual_seed(2)
    v = torch.randn(base.NQ, 3, 3, generator=gen).to(DEV)
    g1, g2 = (torch.randn(base.NQ, 1, 3, generator=gen).to(DEV) for _ in range(2))
    gh = torch.randn(base.NQ, 1, 3, 3, generator=gen).to(DEV)
    one = lambda t: t[:, :, :1].contiguous()
    call = {"directional_nd1": lambda: dec.sample_directional_vjp(rn, q, v[:, 0].contiguous(), gy, one(g1), one(g2), tokens, chunk_points=base.CHUNK),
            "directional_nd1_d2only": lambda: dec.sample_directional_vjp(rn, q, v[:, :1].contiguous(), None, None, one(g2), tokens,
                                                                         chunk_points=base.CHUNK),
            "directional_nd3": lambda: dec.sample_directional_vjp(rn, q, v, gy, g1, g2, tokens, chunk_points=base.CHUNK),
            "directional_nd3_d2only": lambda: dec.sample_directional_vjp(rn, q, v, None, None, g2, tokens, chunk_points=base.CHUNK),
            "hessian": lambda: dec.sample_hessian_vjp(rn, q, gy, gj, gh, tokens, chunk_points=base.CHUNK),
            "hessian_hessonly": lambda: dec.sample_hessian_vjp(rn, q, None, None, gh, tokens, chunk_points=base.CHUNK)}[method]
    dec._stream_grid(rn, q, tokens)                   # the grid's descriptor is found once per token tensor: not part of a call
    torch.cuda.synchronize()
    n0 = ops.launch_count()
    ops.timing_reset(True)
    try:
        call()
        torch.cuda.synchronize()
        return ops.launch_count() - n0, {label: calls for label, (calls, _ms) in sorted(ops.timing_summary().items())}
    finally:
        ops.timing_reset(False)


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("strategy", list(base.STRATEGIES))
def test_a_call_launches_what_it_launched_when_it_arrived(strategy, method):
    from gaot_3d_amd import ops
    got = _profile(strategy, method)
    assert not ops.TIMING["enabled"]
    assert got == EXPECTED[strategy, method], got
    # per chunk: one jet forward and one jet adjoint per scale list, one projection middle
    chunks, lists = -(-base.NQ // base.CHUNK), 1 if strategy == "knn" else 2
    assert sorted(got[1].values()) == sorted([chunks * lists, chunks * lists, chunks]), got
