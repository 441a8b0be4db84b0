"""Model widths the native model accepts besides the shipped 512 x 8 heads (rap_model_create: embed_dim in {256, 512, 768, 1024} with
num_heads = embed_dim / 64, local_feat_dim in {0, 4, ..., 40}, in_dim <= 512): the fixture cases oracle/make_golden.py writes from the
unmodified reference, and the configuration each one is rebuilt from (the fixture stores it)."""
from rap_amd import synthetic as S

WIDTH_CASES = ["w256_ragged_rigid", "w256_latent512_rigid", "w768_emptypart_free", "w768_noqknorm_rigid", "w1024_ragged_rigid"]

# (embed_dim, num_heads) of every accepted width, and the local feature width the few-token / many-token model tests run each one with
WIDTHS = [(256, 4), (512, 8), (768, 12), (1024, 16)]
NEW_WIDTHS = [(256, 4), (768, 12), (1024, 16)]
FEAT_DIM = {256: 4, 512: 32, 768: 12, 1024: 40}


def width_cfg(d, H, layers=2, feat=None, in_dim=0, qk_norm=True):
    cfg = dict(S.RAP_12)
    cfg.update(embed_dim=d, num_heads=H, num_layers=layers, local_feat_dim=FEAT_DIM[d] if feat is None else feat, in_dim=in_dim,
               qk_norm=qk_norm)
    return cfg


def fixture_cfg(g):
    """the configuration a width fixture was generated with"""
    return width_cfg(int(g["embed_dim"]), int(g["num_heads"]), int(g["num_layers"]), int(g["local_feat_dim"]), int(g["in_dim"]),
                     bool(int(g["qk_norm"])))


def fixture_weights(g):
    """-> (cfg, state_dict) of a width fixture; the seeded weights must be the ones it was made with"""
    cfg = fixture_cfg(g)
    sd = S.make_weights(cfg, int(g["weight_seed"]))
    chk = float(sum(v.double().sum().item() for v in sd.values()))
    assert abs(chk - float(g["weights_checksum"])) < 1e-6, "seeded weights differ from the ones the golden was made with"
    return cfg, sd
