"""The launches of the field-sampling API, pinned: for each of the six MAGNODecoder.sample* methods, on a 'knn' decoder (k = 8) and on
a 'bidirectional' one (k = 1, r = 0.9), two scales with softmax weights, C = 32 (one pass of the fused kernels) and C = 48 (two passes,
the last block zero-padded), 70 queries on a 4 x 4 x 4 token grid in chunks of 32 (three chunks, the last one partial; four queries far
outside the box): the number of library launches (ops.launch_count) and the {timing label: calls} map (ops.timing_summary) of one call.
No launch added, none removed, none renamed -- without any timing.  What a C = 48 decoder does is pinned as it is: its projection is
outside the fused jet family (32 -> {64, 128, 256} -> 1..4), so the four second-derivative methods refuse with NotImplementedError
before any launch, and the softmax mix of the scales takes 32 channels only, so the other calls end in its GaotError after the launches
that precede the mix.  C = 48 therefore runs a third time with SUMMED scales, where both passes and the mix complete.

How the literals in EXPECTED were obtained: `_profile` below, as it stands, was run on an MI355X against the package of the commit
BEFORE the host layer was refactored into _fused_passes / _stream_chunks / _mix_scales_jet2 (its parent), and what it returned was pasted
here.  They are not derived from the code under test; a change that moves them has changed what the API launches."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LATENT = (4, 4, 4)
NQ, CHUNK = 70, 32
STRATEGIES = {"knn": 8, "bidirectional": 1}          # decoder strategy -> k_neighbors
METHODS = ("sample", "sample_jacobian", "sample_jacobian_row_lists", "sample_hessian", "sample_laplacian", "sample_hessian_rows",
           "sample_laplacian_rows")                   # the six methods; sample_jacobian without and with row_lists=True

SHAPES = ((32, True), (48, True), (48, False))       # (C, softmax scale weights)
# (strategy, C, weights, method) -> (how the call ended: 'ok' or the exception's type, library launches, {timing label: calls})
EXPECTED = {
    ('knn', 32, True, 'sample'): ('ok', 21, {'gno_fwd_knn_nh2': 3}),
    ('knn', 32, True, 'sample_jacobian'): ('ok', 27, {'gno_fwd_knn_jac_nh2': 3, 'mlp2_jvp_h256_t3': 3}),
    ('knn', 32, True, 'sample_jacobian_row_lists'): ('ok', 27, {'gno_fwd_knn_jac_nh2': 3, 'mlp2_jvp_h256_t3': 3}),
    ('knn', 32, True, 'sample_hessian'): ('ok', 57, {'gno_jet2_knn_nh2_d6': 3, 'mlp2_jet2_h256_d3': 6}),
    ('knn', 32, True, 'sample_laplacian'): ('ok', 36, {'gno_jet2_knn_nh2_d3': 3, 'mlp2_jet2_h256_d3': 3}),
    ('knn', 32, True, 'sample_hessian_rows'): ('ok', 57, {'gno_jet2_knn_nh2_d6': 3, 'mlp2_jet2_h256_d3': 6}),
    ('knn', 32, True, 'sample_laplacian_rows'): ('ok', 36, {'gno_jet2_knn_nh2_d3': 3, 'mlp2_jet2_h256_d3': 3}),
    ('knn', 48, True, 'sample'): ('GaotError', 5, {'gno_fwd_knn_nh2': 2}),
    ('knn', 48, True, 'sample_jacobian'): ('GaotError', 5, {'gno_fwd_knn_jac_nh2': 2}),
    ('knn', 48, True, 'sample_jacobian_row_lists'): ('GaotError', 5, {'gno_fwd_knn_jac_nh2': 2}),
    ('knn', 48, True, 'sample_hessian'): ('NotImplementedError', 0, {}),
    ('knn', 48, True, 'sample_laplacian'): ('NotImplementedError', 0, {}),
    ('knn', 48, True, 'sample_hessian_rows'): ('NotImplementedError', 0, {}),
    ('knn', 48, True, 'sample_laplacian_rows'): ('NotImplementedError', 0, {}),
    ('knn', 48, False, 'sample'): ('ok', 18, {'gno_fwd_knn_nh2': 6}),
    ('knn', 48, False, 'sample_jacobian'): ('ok', 54, {'gno_fwd_knn_jac_nh2': 6}),
    ('knn', 48, False, 'sample_jacobian_row_lists'): ('ok', 54, {'gno_fwd_knn_jac_nh2': 6}),
    ('knn', 48, False, 'sample_hessian'): ('NotImplementedError', 0, {}),
    ('knn', 48, False, 'sample_laplacian'): ('NotImplementedError', 0, {}),
    ('knn', 48, False, 'sample_hessian_rows'): ('NotImplementedError', 0, {}),
    ('knn', 48, False, 'sample_laplacian_rows'): ('NotImplementedError', 0, {}),
    ('bidirectional', 32, True, 'sample'): ('ok', 57, {'gno_fwd_nh2': 6}),
    ('bidirectional', 32, True, 'sample_jacobian'): ('ok', 411, {'gno_bwd_coords_nh2': 6, 'gno_fwd_nh2': 6}),
    ('bidirectional', 32, True, 'sample_jacobian_row_lists'): ('ok', 63, {'gno_fwd_jac_nh2': 6, 'mlp2_jvp_h256_t3': 3}),
    ('bidirectional', 32, True, 'sample_hessian'): ('NotImplementedError', 0, {}),
    ('bidirectional', 32, True, 'sample_laplacian'): ('NotImplementedError', 0, {}),
    ('bidirectional', 32, True, 'sample_hessian_rows'): ('ok', 66, {'gno_jet2_rows_nh2_d6': 6, 'mlp2_jet2_h256_d3': 6}),
    ('bidirectional', 32, True, 'sample_laplacian_rows'): ('ok', 63, {'gno_jet2_rows_nh2_d3': 6, 'mlp2_jet2_h256_d3': 3}),
    ('bidirectional', 48, True, 'sample'): ('GaotError', 20, {'gno_fwd_nh2': 4}),
    ('bidirectional', 48, True, 'sample_jacobian'): ('GaotError', 104, {'gno_fwd_nh2': 4}),
    ('bidirectional', 48, True, 'sample_jacobian_row_lists'): ('GaotError', 20, {'gno_fwd_jac_nh2': 4}),
    ('bidirectional', 48, True, 'sample_hessian'): ('NotImplementedError', 0, {}),
    ('bidirectional', 48, True, 'sample_laplacian'): ('NotImplementedError', 0, {}),
    ('bidirectional', 48, True, 'sample_hessian_rows'): ('NotImplementedError', 0, {}),
    ('bidirectional', 48, True, 'sample_laplacian_rows'): ('NotImplementedError', 0, {}),
    ('bidirectional', 48, False, 'sample'): ('ok', 63, {'gno_fwd_nh2': 12}),
    ('bidirectional', 48, False, 'sample_jacobian'): ('ok', 462, {'gno_bwd_coords_nh2': 12, 'gno_fwd_nh2': 12}),
    ('bidirectional', 48, False, 'sample_jacobian_row_lists'): ('ok', 99, {'gno_fwd_jac_nh2': 12}),
    ('bidirectional', 48, False, 'sample_hessian'): ('NotImplementedError', 0, {}),
    ('bidirectional', 48, False, 'sample_laplacian'): ('NotImplementedError', 0, {}),
    ('bidirectional', 48, False, 'sample_hessian_rows'): ('NotImplementedError', 0, {}),
    ('bidirectional', 48, False, 'sample_laplacian_rows'): ('NotImplementedError', 0, {}),
}


def _decoder(strategy, c, weights):
    from gaot_3d_amd.data import latent_grid
    from gaot_3d_amd.model.layers.magno import MAGNOConfig, MAGNODecoder
    torch.manual_seed(0)
    cfg = MAGNOConfig(gno_coord_dim=3, lifting_channels=c, mlp_type="linear", use_geoembed=[True, False],
                      neighbor_strategy=["knn", strategy], k_neighbors=STRATEGIES[strategy], gno_radius=0.9, scales=[1.0, 2.0],
                      use_scale_weights=weights, out_gno_channel_mlp_hidden_layers=[64, 64], precompute_edges=False)
    dec = MAGNODecoder(in_channels=c, out_channels=1, gno_config=cfg).to(DEV).eval()
    dec.latent_dims = LATENT
    gen = torch.Generator().manual_seed(1)
    tokens = latent_grid(LATENT).to(DEV)
    rn = torch.randn(tokens.shape[0], c, generator=gen).to(DEV)
    q = torch.rand(NQ, 3, generator=gen) * 2.4 - 1.2
    q[-4:] += 5.0                                     # far outside the box
    return dec, rn, q.to(DEV), tokens


def _profile(strategy, c, weights, method):
    """one call of ``method`` -> ('ok' or the type of the exception that ended it, library launches, {timing label: calls})"""
    import gaot_3d_amd
    from gaot_3d_amd import ops
    from gaot_3d_amd._lib import GaotError
    gaot_3d_amd.set_precision("fp32")
    dec, rn, q, tokens = _decoder(strategy, c, weights)
    kw = {"row_lists": True} if method.endswith("_row_lists") else {}
    fn = getattr(dec, method[:-len("_row_lists")] if kw else method)
    dec._stream_grid(rn, q, tokens)                   # the grid's descriptor is found once per token tensor: not part of a call
    torch.cuda.synchronize()
    n0 = ops.launch_count()
    ops.timing_reset(True)
    try:
        how = "ok"
        try:
            fn(rn, q, tokens, chunk_points=CHUNK, **kw)
        except (NotImplementedError, GaotError) as e:
            how = type(e).__name__
        torch.cuda.synchronize()
        return how, ops.launch_count() - n0, {label: calls for label, (calls, _ms) in sorted(ops.timing_summary().items())}
    finally:
        ops.timing_reset(False)


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("c,weights", SHAPES)
@pytest.mark.parametrize("strategy", list(STRATEGIES))
def test_a_call_launches_what_it_launched_before_the_refactor(strategy, c, weights, method):
    from gaot_3d_amd import ops
    got = _profile(strategy, c, weights, method)
    assert not ops.TIMING["enabled"]
    assert got == EXPECTED[strategy, c, weights, method], got
