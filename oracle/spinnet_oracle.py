"""TEST INFRASTRUCTURE ONLY -- restatement of the reference's MiniSpinNet forward (inference; global-z and local-reference-frame modes).

Follows dataset_process/utils/spinnet/patch_embedder.py:49-183, patchnet.py:49-84 and utils/common.py:213-275, 338-372,
387-469 step by step in functional torch (fp32).  pytorch3d 0.7.8 (install.sh:16) is absent: `ball_query_first_k` restates its
documented semantics (first K points of p2, in index order, with squared distance < radius^2; idx padded with -1, neighbours
with zeros) -- parity unpinned for that one function, everything else is pinned to the reference's own modules run in this
container (tests/test_oracle.py::test_spinnet_oracle_matches_live_reference).  Only tests / smoke may import this module.

The default (fp32, CPU) is the path held bit-exact to the reference.  `forward(..., dtype=torch.float64, device=...)` is the same
function in higher precision at sizes the dense tensors of the reference cannot reach: the ball queries are chunked over keypoints,
the convolutions are written as shifted slices + matmul (no backend support for fp64 needed), and an fp64 AMBIGUITY FLAG per
keypoint marks patches in which a discrete decision (in / out of a ball, the choice of the patch normal) is within rounding of
flipping -- there an fp32 implementation may legitimately return the descriptor of the other branch.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

AMBIGUITY_EPS = 2.0 ** -18        # a few tens of fp32 roundings of a three-term sum of squares (fused or not)
LRF_EIGEN_GAP = 1e-3              # relative gap of the two smallest covariance eigenvalues below which the patch normal is ill-defined
LRF_ORIENT_EPS = 1e-6             # |z . centre| <= this * |centre|: the sign of the normal (towards the origin) may flip


def ball_query_first_k(p1, p2, K, radius):
    """p1 (..., P1, 3) queries, p2 (..., P2, 3) -> idx (..., P1, K) long (-1 padded), nn (..., P1, K, 3) (zero padded)"""
    d2 = ((p1[..., :, None, :] - p2[..., None, :, :]) ** 2).sum(-1)
    within = d2 < radius * radius
    rank = within.long().cumsum(-1) - 1
    idx = torch.full(within.shape[:-1] + (K,), -1, dtype=torch.long, device=p1.device)
    nz = torch.nonzero(within & (rank < K), as_tuple=True)                      # (..., query, point)
    idx[nz[:-1] + (rank[nz],)] = nz[-1]
    nn = torch.zeros(idx.shape + (3,), dtype=p2.dtype, device=p2.device)
    nv = torch.nonzero(idx >= 0, as_tuple=True)                                 # (..., query, slot)
    nn[nv] = p2[nv[:-2] + (idx[nv],)]
    return idx, nn


def ball_query_first_k_chunked(p1, p2, K, radius, chunk=256):
    """ball_query_first_k over slices of `chunk` queries: the (P1, P2, 3) difference tensor never exists as a whole"""
    out = [ball_query_first_k(p1[i:i + chunk], p2, K, radius) for i in range(0, p1.shape[0], chunk)]
    return torch.cat([o[0] for o in out]), torch.cat([o[1] for o in out])


def voxel_centres(rad_n=3, azi_n=20, ele_n=7):
    """get_voxel_coordinate(radius=1, ...) (common.py:387-393 with s2_grid :213-225 and change_coordinates :355-372)"""
    beta = np.linspace(0, np.pi, ele_n, endpoint=False) + np.pi / ele_n / 2
    alpha = np.linspace(0, 2 * np.pi, azi_n, endpoint=False) + np.pi / azi_n
    Bm, Am = np.meshgrid(beta, alpha, indexing="ij")
    Bm, Am = Bm.flatten(), Am.flatten()
    s2 = np.stack([np.sin(Bm) * np.cos(Am), np.sin(Bm) * np.sin(Am), np.cos(Bm)], axis=1)
    scale = np.reshape(np.arange(rad_n) / rad_n + 1 / (2 * rad_n), [rad_n, 1, 1])
    return torch.FloatTensor(scale * s2[None]).view(-1, 3)


def bn_eval(x, sd, prefix, affine=True):
    w = sd[prefix + ".weight"] if affine else None
    b = sd[prefix + ".bias"] if affine else None
    return F.batch_norm(x, sd[prefix + ".running_mean"], sd[prefix + ".running_var"], w, b, False, 0.0, 1e-5)


def pad_cyl(x):
    """pad_image / pad_image_3d with kernel 3 (common.py:230-275): circular +-1 on the last (azimuth) axis, zeros +-1 on elevation"""
    x = torch.cat([x[..., -1:], x, x[..., :1]], dim=-1)
    z = torch.zeros_like(x[..., :1, :])
    return torch.cat([z, x, z], dim=-2)


# ---- the same layers as gathers + matmul: any dtype, any device (torch's fp64 convolutions need backend support that is not a given)
def _bn_plain(x, sd, prefix, affine=True):
    shape = (1, -1) + (1,) * (x.dim() - 2)
    y = (x - sd[prefix + ".running_mean"].view(shape)) / torch.sqrt(sd[prefix + ".running_var"].view(shape) + 1e-5)
    return y * sd[prefix + ".weight"].view(shape) + sd[prefix + ".bias"].view(shape) if affine else y


def _conv1x1_plain(x, w, b):
    return torch.einsum("oc,kchw->kohw", w.reshape(w.shape[0], w.shape[1]), x) + b.view(1, -1, 1, 1)


def _conv3x3_plain(xp, w, b):
    """xp (K, C, H+2, W+2) already padded, w (O, C, 3, 3) -> (K, O, H, W): cross-correlation like F.conv2d"""
    H, W = xp.shape[-2] - 2, xp.shape[-1] - 2
    cols = torch.stack([xp[:, :, dy:dy + H, dx:dx + W] for dy in range(3) for dx in range(3)], dim=2)      # (K, C, 9, H, W)
    return torch.einsum("oct,kcthw->kohw", w.reshape(w.shape[0], w.shape[1], 9), cols) + b.view(1, -1, 1, 1)


def _conv3d_plain(xp, w, b):
    """xp (K, C, 3, H+2, W+2), w (O, C, 3, 3, 3), no radial pad -> (K, O, 1, H, W)"""
    H, W = xp.shape[-2] - 2, xp.shape[-1] - 2
    cols = torch.stack([xp[:, :, dz, dy:dy + H, dx:dx + W] for dz in range(3) for dy in range(3) for dx in range(3)], dim=2)
    return (torch.einsum("oct,kcthw->kohw", w.reshape(w.shape[0], w.shape[1], 27), cols) + b.view(1, -1, 1, 1)).unsqueeze(2)


def local_reference_rotation(delta_x, center):
    """cal_Z_axis(disambiguity 'normal') + l2_norm + RodsRotatFormula (common.py:472-496, 539-557) for patches delta_x (K, P, 3)
    centred on `center` (K, 3): z = the singular vector of the smallest singular value of the patch covariance, turned towards the
    origin, and the Rodrigues rotation R with R z = e_z  ->  (R (K,3,3) with p' = R p, ambiguous (K,) bool).  The 3 x 3
    eigen-decomposition runs in fp64 on the CPU whatever the working dtype (the reference's fp32 SVD agrees to rounding whenever
    the smallest singular value is separated)."""
    dt, dev = delta_x.dtype, delta_x.device
    d64 = delta_x.double()
    cov = torch.matmul(d64.transpose(-1, -2), d64).cpu()
    lam, vec = torch.linalg.eigh(cov)                                           # ascending
    z = vec[:, :, 0].clone()
    empty = cov.diagonal(dim1=-2, dim2=-1).sum(-1) == 0                         # 512 copies of the keypoint: svd(0) = I, last column e_z
    z[empty] = torch.tensor([0.0, 0.0, 1.0], dtype=torch.float64)
    c64 = center.double().cpu()
    dot = (z * c64).sum(-1)
    z = torch.where((-dot < 0)[:, None], -z, z)
    z = z / z.norm(dim=1, keepdim=True)
    # (a covariance of numerical rank one -- a single point in the ball -- counts as a tie of its two zero eigenvalues)
    ambiguous = (~empty & ((lam[:, 1] - lam[:, 0]) <= LRF_EIGEN_GAP * torch.maximum(lam[:, 1], 1e-9 * lam[:, 2]))) | \
                (~empty & (c64.norm(dim=1) > 0) & (dot.abs() <= LRF_ORIENT_EPS * c64.norm(dim=1)))
    ez = torch.tensor([0.0, 0.0, 1.0], dtype=torch.float64).expand_as(z)
    c = F.normalize(torch.cross(z, ez, dim=1), p=2, dim=1)
    theta = torch.acos(z[:, 2].clamp(-1, 1))[:, None, None]
    Kx = torch.zeros(z.shape[0], 3, 3, dtype=torch.float64)
    Kx[:, 0, 1] = -c[:, 2]; Kx[:, 0, 2] = c[:, 1]; Kx[:, 1, 0] = c[:, 2]; Kx[:, 1, 2] = -c[:, 0]; Kx[:, 2, 0] = -c[:, 1]; Kx[:, 2, 1] = c[:, 0]
    R = torch.eye(3, dtype=torch.float64)[None] + torch.sin(theta) * Kx + (1 - torch.cos(theta)) * torch.matmul(Kx, Kx)
    return R.to(device=dev, dtype=dt), ambiguous.to(dev)


def _ball_ambiguity(kpts64, p64, des_r, chunk):
    """a cloud point with | |p - kpt|^2 - r^2 | <= eps r^2"""
    r2 = float(des_r) * float(des_r)
    out = []
    for i in range(0, kpts64.shape[0], chunk):
        d2 = ((kpts64[i:i + chunk, None, :] - p64[None, :, :]) ** 2).sum(-1)
        out.append(((d2 - r2).abs() <= AMBIGUITY_EPS * r2).any(dim=1))
    return torch.cat(out)


def _voxel_ambiguity(vox64, q64):
    """a (voxel centre v, patch point q) pair with | |v - q|^2 - (0.8/3)^2 | <= eps (|v|^2 + |q|^2); q64 (B, 512, 3)"""
    vr2 = (0.8 / 3) ** 2
    d2 = ((vox64[None, :, None, :] - q64[:, None, :, :]) ** 2).sum(-1)                         # (B, 420, 512)
    scale = (vox64 ** 2).sum(-1)[None, :, None] + (q64 ** 2).sum(-1)[:, None, :]
    return ((d2 - vr2).abs() <= AMBIGUITY_EPS * scale).flatten(1).any(dim=1)


def forward(sd, pts, kpts, des_r, perm, dtype=torch.float32, device="cpu", lrf=False, chunk=64):
    """pts (N,3), kpts (K,3), perm (N,) -> desc (K,32); intermediates (`patches`, `x0`, `equi_raw`, `ball_counts`) and the per-keypoint
    `ambiguous` flag in a dict for stage-wise checks.  `lrf` = not is_aligned_to_global_z.  `chunk` keypoints are in flight at a time."""
    device = torch.device(device)
    plain = dtype != torch.float32 or device.type != "cpu"       # the fp32 CPU path keeps torch's own layers (bit-pinned to the reference)
    sd = {k: v.to(device=device, dtype=dtype) for k, v in sd.items()}
    pts = pts.to(device=device, dtype=dtype); kpts = kpts.to(device=device, dtype=dtype)
    p = pts[torch.as_tensor(perm, dtype=torch.long, device=device)]             # patch_embedder.py:99-100
    Kn = kpts.shape[0]
    idx, nn = ball_query_first_k_chunked(kpts, p, 512, des_r, chunk=256)        # :104-110
    invalid = (idx == -1).to(dtype)[..., None]
    patch = nn * (1 - invalid) + kpts[:, None, :] * invalid                     # :122-131
    center = patch[:, -1, :]                                                    # :142
    delta = patch - center[:, None, :]                                          # :143
    ambiguous = _ball_ambiguity(kpts.double(), p.double(), des_r, 256)
    if lrf:                                                                     # :145-152
        Rm, amb_axis = local_reference_rotation(delta, center)
        delta = torch.matmul(delta, Rm.transpose(-1, -2))
        ambiguous = ambiguous | amb_axis
    delta = delta / des_r                                                       # :185-188
    vox = voxel_centres().to(device=device, dtype=dtype)
    ang = -torch.arange(20, dtype=torch.float64) * (2 * np.pi / 20)             # var_to_invar, common.py:443-469
    R = torch.zeros(20, 3, 3, dtype=torch.float64)
    R[:, 0, 0] = torch.cos(ang); R[:, 0, 1] = -torch.sin(ang); R[:, 1, 0] = torch.sin(ang); R[:, 1, 1] = torch.cos(ang); R[:, 2, 2] = 1
    R = R.float().to(device=device, dtype=dtype)
    bn = _bn_plain if plain else bn_eval
    x0s, xs, descs, amb_vox = [], [], [], []
    for k0 in range(0, Kn, chunk):
        dk = delta[k0:k0 + chunk]
        Kc = dk.shape[0]
        amb_vox.append(_voxel_ambiguity(vox.double(), dk.double()))
        gi, sn = ball_query_first_k(vox[None].expand(Kc, -1, -1), dk, 10, 0.8 / 3)             # sphere_query, common.py:396-440
        mask = (gi == gi[..., :1]).to(dtype); mask[..., 0] = 0
        mask[..., 0] += (gi[..., 0] == 0).to(dtype)
        samples = sn * (1 - mask[..., None])                                    # (Kc, 420, 10, 3)
        s = samples.view(Kc, 3, 7, 20, 10, 3)
        inv = torch.matmul(s, R.transpose(-1, -2)[None, None, None]).view(Kc, 420, 10, 3)
        x = inv.permute(0, 3, 1, 2)                                             # (K,3,420,10)  patch_embedder.py:74
        if plain:
            x = F.relu(bn(_conv1x1_plain(x, sd["pnt_layer.0.weight"], sd["pnt_layer.0.bias"]), sd, "pnt_layer.1"))
        else:
            x = F.relu(bn(F.conv2d(x, sd["pnt_layer.0.weight"], sd["pnt_layer.0.bias"]), sd, "pnt_layer.1"))
        x = x.max(dim=3).values.view(Kc, 16, 3, 7, 20)                          # :76-78
        x0s.append(x)
        if plain:                                                               # patchnet.py:52-61
            x = _conv3d_plain(pad_cyl(x), sd["conv_net.ops.0.weight"], sd["conv_net.ops.0.bias"])
        else:
            x = F.conv3d(pad_cyl(x), sd["conv_net.ops.0.weight"], sd["conv_net.ops.0.bias"])
        x = F.relu(bn(x, sd, "conv_net.ops.1", affine=False)).squeeze(2)
        for i in range(1, 8):
            op = 3 * i
            conv = _conv3x3_plain if plain else F.conv2d
            x = conv(pad_cyl(x), sd[f"conv_net.ops.{op}.weight"], sd[f"conv_net.ops.{op}.bias"])
            if i < 7:
                x = F.relu(bn(x, sd, f"conv_net.ops.{op + 1}", affine=False))
        c1 = _conv1x1_plain if plain else F.conv2d
        w = F.relu(bn(c1(x, sd["pool_layer.0.weight"], sd["pool_layer.0.bias"]), sd, "pool_layer.1"))
        w = F.relu(bn(c1(w, sd["pool_layer.3.weight"], sd["pool_layer.3.bias"]), sd, "pool_layer.4"))
        f = (x * w).mean(dim=(2, 3))                                            # patch_embedder.py:82
        descs.append(F.normalize(f, p=2, dim=1))
        xs.append(x)
    cat = lambda ts, shape: torch.cat(ts) if ts else torch.zeros(shape, dtype=dtype, device=device)
    if Kn:
        ambiguous = ambiguous | torch.cat(amb_vox)
    return {"desc": cat(descs, (0, 32)), "patches": delta, "x0": cat(x0s, (0, 16, 3, 7, 20)), "equi_raw": cat(xs, (0, 32, 7, 20)),
            "ball_counts": (idx >= 0).sum(dim=1), "ambiguous": ambiguous}
