"""CPU: every model width the native model accepts (embed_dim 256 / 512 / 768 / 1024, num_heads = embed_dim / 64): the oracle against
fixtures of the unmodified reference at the other widths, the native weight count against the reference's parameter layout over the
whole accepted envelope, and the configurations outside it refused by the library and by PointCloudDiT."""
import ctypes
import math

import pytest
import torch

import rap_amd
from conftest import load_golden
from oracle import rap_oracle as O
from rap_amd import _lib
from rap_amd import synthetic as S
from width_cases import WIDTH_CASES, WIDTHS, fixture_weights


@pytest.mark.parametrize("name", WIDTH_CASES)
def test_oracle_matches_reference_golden_at_other_widths(name):
    g, inp = load_golden(name)
    cfg, sd = fixture_weights(g)
    assert sd["encoding_manager.emb_proj.weight"].shape == (cfg["embed_dim"], S.embed_in_dim(cfg))
    assert inp["features"].shape[1] == cfg["local_feat_dim"]
    out = O.sample(sd, cfg, inp, int(g["num_steps"]), bool(g["rigidity"]))
    for k in ("end_point_trajectory", "trajectory", "R", "t"):
        err = float((out[k] - torch.from_numpy(g[k])).abs().max())
        assert err < 5e-6, (k, err)
    f_ref = torch.from_numpy(g["sample_features"])
    assert f_ref.shape[1] == cfg["embed_dim"]
    assert float(g["sample_features_timestep"]) == pytest.approx(1.0 / int(g["num_steps"]))
    assert float((out["transformer_features"] - f_ref).abs().max()) < 2e-5 * max(1.0, float(f_ref.abs().max()))
    cu_b, cu_p = O.prepare_cu_seqlens(inp)
    fw = O.dit_forward(sd, cfg, inp["x_1"], torch.from_numpy(g["fwd_timesteps"]), inp["pointclouds"], inp["features"],
                       inp["scales"], inp["anchor_indices"], cu_b, cu_p, return_transformer_features=True, latent=inp.get("latent_features"))
    assert float((fw["velocity"] - torch.from_numpy(g["fwd_velocity"])).abs().max()) < 2e-6
    assert float((fw["transformer_features"] - torch.from_numpy(g["fwd_features"])).abs().max()) < 2e-5


@pytest.mark.parametrize("d,H", WIDTHS)
def test_weight_count_matches_the_reference_layout_at_every_accepted_width(d, H):
    lib = _lib.load()
    for feat in range(0, 44, 4):
        for in_dim in (0, 64, 512):
            cfg = dict(embed_dim=d, num_heads=H, num_layers=2, local_feat_dim=feat, in_dim=in_dim)
            desc = _lib.ModelDesc(d, 2, H, feat)
            n = lib.rap_weight_count_latent(ctypes.byref(desc), in_dim)
            assert n == sum(math.prod(s) for _, s in S.weight_spec(cfg)), (d, feat, in_dim)


# (embed_dim, num_heads, local_feat_dim, in_dim) outside the accepted envelope: widths not a multiple of 256 or above 1024, heads other
# than embed_dim / 64, feature widths not a multiple of 4 or above 40, latent widths above 512
REFUSED = [(128, 2, 32, 0), (384, 6, 32, 0), (1280, 20, 32, 0), (512, 4, 32, 0), (256, 8, 4, 0), (1024, 8, 40, 0),
           (512, 8, 6, 0), (512, 8, 44, 0), (256, 4, 4, 516)]


@pytest.mark.parametrize("d,H,feat,in_dim", REFUSED)
def test_configurations_outside_the_envelope_are_refused(d, H, feat, in_dim):
    lib = _lib.load()
    desc = _lib.ModelDesc(d, 2, H, feat)
    assert lib.rap_weight_count_latent(ctypes.byref(desc), in_dim) < 0
    with pytest.raises(NotImplementedError):
        rap_amd.PointCloudDiT(in_dim=in_dim, out_dim=3, embed_dim=d, num_layers=2, num_heads=H, local_feat_dim=feat)
