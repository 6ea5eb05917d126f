"""The launches of the field ADJOINTS, pinned: for each of the three MAGNODecoder.sample*_vjp methods, on a 'knn' decoder (k = 8) and on
a 'bidirectional' one (k = 1, r = 0.9), two scales with softmax weights, C = 32 (one pass of the fused kernels) and C = 48 (two passes,
the last block zero-padded), 70 queries on a 4 x 4 x 4 token grid in chunks of 32 (three chunks, the last one partial; four queries far
outside the box): the number of library launches (ops.launch_count) and the {timing label: calls} map (ops.timing_summary) of one call.
sample_jacobian_vjp runs with cot_pred given and with cot_pred=None, sample_laplacian_vjp with all three cotangents and with
cot_pred=cot_jac=None; the cotangents come from a seeded CPU generator.  No launch added, none removed, none renamed -- without any
timing.  What a C = 48 decoder does is pinned as it is (a refusal before any launch, or the GaotError of the 32-channel softmax mix
after the launches that precede it); C = 48 runs a third time with SUMMED scales.

How the literals in EXPECTED were obtained: `_profile` below, as it stands, was run on an MI355X against the package of the commit
BEFORE the three adjoint host paths were folded into one driver (its parent), and what it returned was pasted here.  They are not
derived from the code under test; a change that moves them has changed what the API launches."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LATENT = (4, 4, 4)
NQ, CHUNK = 70, 32
STRATEGIES = {"knn": 8, "bidirectional": 1}          # decoder strategy -> k_neighbors
# the three methods; sample_jacobian_vjp also without cot_pred, sample_laplacian_vjp also with cot_lap alone
METHODS = ("sample_vjp", "sample_jacobian_vjp", "sample_jacobian_vjp_nopred", "sample_laplacian_vjp", "sample_laplacian_vjp_laponly")

SHAPES = ((32, True), (48, True), (48, False))       # (C, softmax scale weights)
# (strategy, C, weights, method) -> (how the call ended: 'ok' or the exception's type, library launches, {timing label: calls})
EXPECTED = {
    ('knn', 32, True, 'sample_vjp'): ('ok', 69, {'gno_adj_nh2': 3, 'gno_fwd_knn_nh2': 3}),
    ('knn', 32, True, 'sample_jacobian_vjp'): ('ok', 84, {'gno_adj_jac_nh2': 3, 'gno_fwd_knn_jac_nh2': 3}),
    ('knn', 32, True, 'sample_jacobian_vjp_nopred'): ('ok', 84, {'gno_adj_jac_nh2': 3, 'gno_fwd_knn_jac_nh2': 3}),
    ('knn', 32, True, 'sample_laplacian_vjp'): ('ok', 99, {'gno_adj_jet2_nh2': 3, 'gno_jet2_knn_nh2_d3': 3, 'mlp2_lap_cot_mid_h256': 3}),
    ('knn', 32, True, 'sample_laplacian_vjp_laponly'): ('ok', 99, {'gno_adj_jet2_nh2': 3, 'gno_jet2_knn_nh2_d3': 3, 'mlp2_lap_cot_mid_h256': 3}),
    ('knn', 48, True, 'sample_vjp'): ('GaotError', 5, {'gno_fwd_knn_nh2': 2}),
    ('knn', 48, True, 'sample_jacobian_vjp'): ('GaotError', 5, {'gno_fwd_knn_jac_nh2': 2}),
    ('knn', 48, True, 'sample_jacobian_vjp_nopred'): ('GaotError', 5, {'gno_fwd_knn_jac_nh2': 2}),
    ('knn', 48, True, 'sample_laplacian_vjp'): ('NotImplementedError', 0, {}),
    ('knn', 48, True, 'sample_laplacian_vjp_laponly'): ('NotImplementedError', 0, {}),
    ('knn', 48, False, 'sample_vjp'): ('ok', 66, {'gno_adj_nh2': 6, 'gno_fwd_knn_nh2': 6}),
    ('knn', 48, False, 'sample_jacobian_vjp'): ('ok', 81, {'gno_adj_jac_nh2': 6, 'gno_fwd_knn_jac_nh2': 6}),
    ('knn', 48, False, 'sample_jacobian_vjp_nopred'): ('ok', 81, {'gno_adj_jac_nh2': 6, 'gno_fwd_knn_jac_nh2': 6}),
    ('knn', 48, False, 'sample_laplacian_vjp'): ('NotImplementedError', 0, {}),
    ('knn', 48, False, 'sample_laplacian_vjp_laponly'): ('NotImplementedError', 0, {}),
    ('bidirectional', 32, True, 'sample_vjp'): ('ok', 132, {'gno_adj_nh2': 6, 'gno_fwd_nh2': 6}),
    ('bidirectional', 32, True, 'sample_jacobian_vjp'): ('ok', 150, {'gno_adj_jac_nh2': 6, 'gno_fwd_jac_nh2': 6}),
    ('bidirectional', 32, True, 'sample_jacobian_vjp_nopred'): ('ok', 150, {'gno_adj_jac_nh2': 6, 'gno_fwd_jac_nh2': 6}),
    ('bidirectional', 32, True, 'sample_laplacian_vjp'): ('ok', 153, {'gno_adj_jet2_nh2': 6, 'gno_jet2_rows_nh2_d3': 6, 'mlp2_lap_cot_mid_h256': 3}),
    ('bidirectional', 32, True, 'sample_laplacian_vjp_laponly'): ('ok', 153, {'gno_adj_jet2_nh2': 6, 'gno_jet2_rows_nh2_d3': 6, 'mlp2_lap_cot_mid_h256': 3}),
    ('bidirectional', 48, True, 'sample_vjp'): ('GaotError', 20, {'gno_fwd_nh2': 4}),
    ('bidirectional', 48, True, 'sample_jacobian_vjp'): ('GaotError', 20, {'gno_fwd_jac_nh2': 4}),
    ('bidirectional', 48, True, 'sample_jacobian_vjp_nopred'): ('GaotError', 20, {'gno_fwd_jac_nh2': 4}),
    ('bidirectional', 48, True, 'sample_laplacian_vjp'): ('NotImplementedError', 0, {}),
    ('bidirectional', 48, True, 'sample_laplacian_vjp_laponly'): ('NotImplementedError', 0, {}),
    ('bidirectional', 48, False, 'sample_vjp'): ('ok', 147, {'gno_adj_nh2': 12, 'gno_fwd_nh2': 12}),
    ('bidirectional', 48, False, 'sample_jacobian_vjp'): ('ok', 153, {'gno_adj_jac_nh2': 12, 'gno_fwd_jac_nh2': 12}),
    ('bidirectional', 48, False, 'sample_jacobian_vjp_nopred'): ('ok', 153, {'gno_adj_jac_nh2': 12, 'gno_fwd_jac_nh2': 12}),
    ('bidirectional', 48, False, 'sample_laplacian_vjp'): ('NotImplementedError', 0, {}),
    ('bidirectional', 48, False, 'sample_laplacian_vjp_laponly'): ('NotImplementedError', 0, {}),
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
    cots = [torch.randn(NQ, 1, *tail, generator=gen).to(DEV) for tail in ((), (3,), ())]      # cot_pred, cot_jac, cot_lap
    return dec, rn, q.to(DEV), tokens, cots


def _profile(strategy, c, weights, method):
    """one call of ``method`` -> ('ok' or the type of the exception that ended it, library launches, {timing label: calls})"""
    import gaot_3d_amd
    from gaot_3d_amd import ops
    from gaot_3d_amd._lib import GaotError
    gaot_3d_amd.set_precision("fp32")
    dec, rn, q, tokens, (gy, gj, gl) = _decoder(strategy, c, weights)
    name, cots = {"sample_vjp": ("sample_vjp", (gy,)),
                  "sample_jacobian_vjp": ("sample_jacobian_vjp", (gy, gj)),
                  "sample_jacobian_vjp_nopred": ("sample_jacobian_vjp", (None, gj)),
                  "sample_laplacian_vjp": ("sample_laplacian_vjp", (gy, gj, gl)),
                  "sample_laplacian_vjp_laponly": ("sample_laplacian_vjp", (None, None, gl))}[method]
    fn = getattr(dec, name)
    dec._stream_grid(rn, q, tokens)                   # the grid's descriptor is found once per token tensor: not part of a call
    torch.cuda.synchronize()
    n0 = ops.launch_count()
    ops.timing_reset(True)
    try:
        how = "ok"
        try:
            fn(rn, q, *cots, tokens, chunk_points=CHUNK)
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
