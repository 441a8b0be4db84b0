"""GPU: edge sweep of the kernels either side of the sampler -- raw scans to the packed batch, predicted poses to transform matrices, RRE /
RTE figures and the selected generation -- against plain float64 references on the same inputs (inputs, references and bounds:
tests/boundary_cases.py, checked by tests/test_boundary_cases_host.py).

test -> kernel -> edge
  test_collate_part_sizes ............ collate_part_sums_kernel, collate_frame_kernel: parts of 1 .. 70001 points, each once primary and once
                                        not (256-thread stride loops, wave edges, the four-wave staging array); collate_apply_kernel: TP not a
                                        multiple of 256, a random order, features gathered with the points
  test_collate_primary_part .......... collate_frame_kernel: the first arg-max at column 0, inside, at P-1, ties of two and three and of the
                                        last two; the extent-defining point at index 0, 63, 64, 255, 256, n-1 (block max), negative extremes;
                                        the reference's own np.random.permutation draws
  test_collate_part_counts ........... collate_frame_kernel `threadIdx.x < P` at P = 1 .. 256 (every thread at 256), trailing padding;
                                        collate_apply_kernel binary search over B*P up to 16640 parts with runs of empty ones; B = 1, 2, 65
  test_collate_refusals .............. rap_collate_transform: P = 257, B*P = 65536, a workspace one byte short (return values, nothing written)
  test_collate_empty_parts ........... (C ABI) collate_apply_kernel binary search over empty parts in front and inside; part columns kept; a
                                        sample of empty parts only between two normal ones
  test_collate_order_is_checked ...... collate_check_order_kernel: the off-by-one at n (last point of the last part), -1 at point 0, a
                                        valid order not flagged; the clamp of collate_apply_kernel (nothing outside the part is read)
  test_collate_input_types ........... load_pt: fp64 clouds 1e5 out, fp32 clouds 3e2 out, one fp64 part promoting the batch
  test_collate_single_point_primary .. collate_frame_kernel / collate_apply_kernel: scale 0, the oracle's finite / non-finite pattern
  test_relative_transforms ........... relative_transform_kernel: B*P from 1 to 260 (second .. fifth block, b = i / P across the block edge),
                                        empty parts at lanes 63 / 64, no / rigid / general global frame (adjugate against a general inverse)
  test_transform_errors .............. transform_errors_kernel: the `p += 64` loop (P = 65, 130), anchor first / inside / last / twice / absent
                                        / alone / on an empty part, matched ids incl. out-of-range ones (clamp), eight error angles on both
                                        sides of column 64
  test_transform_errors_direct ....... transform_errors_direct_kernel: the same cases without the anchor frame
  test_argmin_generation ............. argmin_generation_kernel: B = 1 .. 200 (second to fourth block), G = 1 .. 17, ties, +-inf and NaN on
                                        both sides of sample 64, both pick_largest settings, clouds = NULL
  test_gather_generation ............. gather_generation_kernel: samples of 0 .. 5000 points around 256 floats and the 16 x 256-float stride,
                                        the `i += 256` loops over P*9 and P*3 (P = 28, 29, 86), a 65-sample batch
  test_token_sample .................. token_sample_kernel: B = 1 and 1000, empty samples first / inside / last / in a row, lengths around the
                                        64 x 256 grid stride, nothing written outside [cu[0], cu[B])
  test_check_batch ................... check_batch_kernel: every documented bit by its minimal defect, alone where it can be, combinations
"""
import ctypes

import numpy as np
import pytest
import torch

import boundary_cases as BC
import guards as G
import rap_amd
from rap_amd import _lib, evaluator, metrics, selection

pytestmark = pytest.mark.gpu

RAP_ERR_INVALID, RAP_ERR_WORKSPACE = -1, -2
VP = ctypes.c_void_p


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def stream(dev):
    return _lib.current_stream(dev)


# ---------------------------------------------------------------------------------------------
# 1. collate
# ---------------------------------------------------------------------------------------------
def run_wrapper(batch, dev):
    samples = BC.as_samples(batch)
    if batch["order"] == "numpy":
        np.random.seed(batch["np_seed"])
        return rap_amd.transform_and_collate(samples, batch["P"], shuffle=True, device=dev)
    if batch["order"] == "none":
        return rap_amd.transform_and_collate(samples, batch["P"], shuffle=False, device=dev)
    return rap_amd.transform_and_collate(samples, batch["P"], order=BC.flat_order(batch), device=dev)


OUTPUTS = (("pointclouds", torch.float32, 3), ("pointclouds_gt", torch.float32, 3), ("features", torch.float32, None),
           ("anchor_indices", torch.uint8, 1), ("part_indices", torch.int64, 1))


def run_abi(lib, dev, batch, order="batch", B=None, P=None, ws_short=0):
    """rap_collate_transform itself, every output and the workspace inside guard bands, the workspace of exactly the queried size.
    -> (return code, dict of numpy arrays, order flag, the guarded buffers)"""
    counts = batch["counts"]
    B, P = (counts.shape[0] if B is None else B), (counts.shape[1] if P is None else P)
    f64 = any(x.dtype == np.float64 for x in batch["parts"])
    pts = torch.from_numpy(np.concatenate([x.astype(np.float64 if f64 else np.float32) for x in batch["parts"]])).to(dev)
    TP, F = pts.shape[0], batch["F"]
    feat = torch.from_numpy(np.concatenate(batch["feats"])).to(dev) if F > 0 else None
    order = (BC.flat_order(batch) if isinstance(order, str) else order)
    order = None if order is None else order.to(dev)
    ppp = torch.from_numpy(counts).to(dev)
    bufs, views = {}, {}

    def out(name, dtype, shape):
        n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
        bufs[name] = G.Guarded(max(n, 1), dev, name=name)
        views[name] = bufs[name].view(dtype, shape)
        return _lib.ptr(views[name]) if n else None

    nB, nP = counts.shape
    ptrs = [out(k, dt, (TP, F if w is None else w)) for k, dt, w in OUTPUTS]
    tabs = [out("rotations", torch.float32, (nB, nP, 3, 3)), out("translations", torch.float32, (nB, nP, 3)), out("scales", torch.float32, (nB,)),
            out("anchor_parts", torch.uint8, (nB, nP)), out("global_translation", torch.float32, (nB, 3)), out("cu_seqlens", torch.int64, (nB + 1,))]
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    need = lib.rap_collate_workspace_bytes(nB, nP)
    bufs["workspace"] = G.Guarded(need, dev, name="workspace")
    rc = lib.rap_collate_transform(_lib.ptr(pts), 1 if f64 else 0, _lib.ptr(ppp), B, P, TP, _lib.ptr(order), _lib.ptr(feat), F, ptrs[0], ptrs[1],
                                   ptrs[2] if F else None, ptrs[3], ptrs[4], *tabs, _lib.ptr(flag), VP(bufs["workspace"].ptr), need - ws_short,
                                   stream(dev))
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy().copy() for k, v in views.items()}
    for k in ("anchor_indices", "part_indices"):
        got[k] = got[k].reshape(-1)
    got["points_per_part"] = counts
    return rc, got, int(flag.item()), bufs


def assert_collate(got, exp, name, F):
    """integer and boolean keys bit-equal, feature rows bit-equal, float keys within one fp32 ulp (BC.collate_tolerance) wherever the
    reference is finite and the same finite / non-finite pattern"""
    for k in BC.COLLATE_EXACT_KEYS:
        if k == "features" and F == 0:
            continue
        g = got[k].cpu().numpy() if isinstance(got[k], torch.Tensor) else got[k]
        assert g.shape == exp[k].shape, (name, k, g.shape, exp[k].shape)
        assert np.array_equal(g.astype(exp[k].dtype), exp[k]), (name, k)
    worst = {}
    for k in BC.COLLATE_FLOAT_KEYS:
        g = (got[k].cpu().numpy() if isinstance(got[k], torch.Tensor) else got[k]).astype(np.float64)
        assert g.shape == exp[k].shape, (name, k, g.shape, exp[k].shape)
        fin = np.isfinite(exp[k])
        assert np.array_equal(np.isfinite(g), fin), (name, k, "finite / non-finite pattern")
        ratio = np.abs(g - exp[k].astype(np.float64))[fin] / BC.collate_tolerance(exp[k])[fin]
        worst[k] = float(ratio.max()) if ratio.size else 0.0
    print(f"collate {name}: worst error in fp32 ulp (bound 1) " + ", ".join(f"{k} {v:.2f}" for k, v in worst.items()))
    assert max(worst.values()) <= 1.0, (name, worst)


def test_collate_part_sizes(dev):
    b = BC.collate_sizes_batch()
    exp = BC.collate_expected(b)
    got = run_wrapper(b, dev)
    assert got["num_parts"] == [int((r > 0).sum()) for r in b["counts"]]
    # sample 0 is two one-point parts: its scale is 0 and the oracle's division gives non-finite values there, and only there
    assert float(got["scales"][0]) == 0.0 and bool(torch.isfinite(got["pointclouds"][2:]).all())
    assert_collate(got, exp, "sizes", b["F"])


def test_collate_primary_part(dev):
    b = BC.collate_primary_batch()
    exp = BC.collate_expected(b)
    got = run_wrapper(b, dev)
    assert_collate(got, exp, "primary", b["F"])
    assert got["anchor_parts"].cpu().numpy().argmax(1)[:6].tolist() == [0, 1, 4, 0, 0, 1]
    # the scale is 1.5 x the one coordinate that was moved out: the block maximum found it wherever it sat
    k = int((b["counts"][:6] > 0).sum())
    for j, (sample, idx, axis, sign) in enumerate(b["extent"]):
        part = b["parts"][k + 2 * j + 1]
        want = 1.5 * abs(part[idx, axis] - part[:, axis].mean())
        assert abs(float(got["scales"][sample]) - want) <= BC.F32_ULP * max(1.0, want), (sample, idx)


@pytest.mark.parametrize("P,B", BC.PART_COUNT_SHAPES)
def test_collate_part_counts(dev, P, B):
    b = BC.collate_part_count_batches()[(P, B)]
    assert_collate(run_wrapper(b, dev), BC.collate_expected(b), f"P={P} B={B}", 0)


def test_collate_refusals(lib, dev):
    """return values only: nothing is launched and no output byte changes"""
    b = BC.collate_part_count_batches()[(2, 2)]
    for kw, want in ((dict(P=257), RAP_ERR_INVALID), (dict(B=256, P=256), RAP_ERR_INVALID), (dict(ws_short=1), RAP_ERR_WORKSPACE)):
        rc, _, flag, bufs = run_abi(lib, dev, b, **kw)
        assert rc == want and flag == 0, (kw, rc)
        for g in bufs.values():
            g.check()
            assert g.untouched(), (kw, g.name)
    assert lib.rap_collate_workspace_bytes(256, 256) > 0 and 256 * 256 == 65536
    rc, got, flag, bufs = run_abi(lib, dev, b)                               # the same call, unchanged, is accepted
    assert rc == 0 and flag == 0
    assert_collate(got, BC.collate_expected(b), "C ABI P=2 B=2", 0)


def test_collate_empty_parts(lib, dev):
    b = BC.collate_empty_parts_batch()
    exp = BC.collate_expected(b)
    rc, got, flag, bufs = run_abi(lib, dev, b)
    assert rc == 0 and flag == 0
    for g in bufs.values():
        g.check()
    assert_collate(got, exp, "empty parts", b["F"])
    # the sample without a point: scale 0, global translation 0, zero rows, no anchor, a repeated cu_seqlens entry
    assert got["scales"][2] == 0 and not got["global_translation"][2].any() and not got["rotations"][2].any() and not got["translations"][2].any()
    assert not got["anchor_parts"][2].any() and got["cu_seqlens"][2] == got["cu_seqlens"][3]


def test_collate_order_is_checked(lib, dev):
    b = BC.collate_single_point_batch()
    samples, P = BC.as_samples(b), b["P"]
    good = BC.flat_order(b)
    n_last = int(b["counts"][-1][b["counts"][-1] > 0][-1])
    for pos, val in ((-1, n_last), (0, -1), (0, int(b["counts"][0, 0]))):
        bad = good.clone()
        bad[pos] = val
        with pytest.raises(ValueError):
            rap_amd.transform_and_collate(samples, P, order=bad, device=dev)
    bad = good.clone()
    bad[-1] = n_last - 1                                                     # the largest index of the part is in range (here a duplicate: not checked)
    rap_amd.transform_and_collate(samples, P, order=bad, device=dev)
    rap_amd.transform_and_collate(samples, P, order=good, device=dev)
    # an index outside its part is clamped into it before it is used: with the points inside guard bands of two different contents the
    # outputs are the same, and they are those of the clamped order
    bad = good.clone()
    bad[-1], bad[0] = n_last, -1
    clamped = good.clone()
    clamped[-1], clamped[0] = n_last - 1, 0
    rc, got, flag, _ = run_abi(lib, dev, b, order=bad)
    rc2, want, flag2, _ = run_abi(lib, dev, b, order=clamped)
    assert (rc, flag, rc2, flag2) == (0, 1, 0, 0)
    for k in ("pointclouds", "pointclouds_gt", "features"):
        assert np.array_equal(got[k], want[k], equal_nan=True), k


@pytest.mark.parametrize("kind", ["f64_far", "f32", "mixed"])
def test_collate_input_types(dev, kind):
    b = BC.collate_dtype_batches()[kind]
    assert_collate(run_wrapper(b, dev), BC.collate_expected(b), kind, b["F"])


def test_collate_single_point_primary(dev):
    b = BC.collate_single_point_batch()
    exp = BC.collate_expected(b)
    got = run_wrapper(b, dev)
    assert_collate(got, exp, "single-point primary", b["F"])
    cu = exp["cu_seqlens"]
    assert float(got["scales"][1]) == 0.0 and not bool(torch.isfinite(got["pointclouds_gt"][cu[1]:cu[2]]).any())
    alone = [dict(b, counts=b["counts"][s:s + 1], parts=b["parts"][k0:k1], feats=b["feats"][k0:k1], perms=b["perms"][k0:k1])
             for s, k0, k1 in ((0, 0, 2), (2, 5, 8))]
    for s, a in zip((0, 2), alone):                                            # the neighbours are bit for bit what they are alone
        ga = run_wrapper(a, dev)
        assert torch.equal(ga["pointclouds"], got["pointclouds"][cu[s]:cu[s + 1]]) and torch.equal(ga["translations"][0], got["translations"][s])


# ---------------------------------------------------------------------------------------------
# 2. output transforms
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("frame", BC.REL_FRAMES)
@pytest.mark.parametrize("B,P", BC.REL_SHAPES)
def test_relative_transforms(dev, B, P, frame):
    c = BC.relative_case(B, P)
    Gr, gt = BC.relative_frame(c, frame)
    ref, bound = BC.relative_transforms_f64(c["R_pred"], c["t_pred"], c["R_gt"], c["t_gt"], c["scales"], c["ppp"], Gr, gt)
    out = evaluator.compute_relative_transforms(c["R_pred"].to(dev), c["t_pred"], c["R_gt"], c["t_gt"], c["scales"], c["ppp"], Gr, gt)
    got = out.cpu().double().numpy()
    empty = (c["ppp"] == 0).numpy()
    assert not got[empty].any()                                                                  # all-zero 4x4 blocks, bit for bit
    assert (got[~empty][:, 3] == np.array([0.0, 0.0, 0.0, 1.0])).all()
    err = np.abs(got - ref)
    print(f"relative transforms B={B} P={P} {frame}: worst error / bound {float((err[bound > 0] / bound[bound > 0]).max()):.3f}, "
          f"largest entry {np.abs(ref).max():.3g}")
    assert (err <= bound).all(), (B, P, frame, float((err - bound).max()))


# ---------------------------------------------------------------------------------------------
# 3. transform errors
# ---------------------------------------------------------------------------------------------
def _nan_mask_equal(got, ref):
    return torch.equal(torch.isnan(got), torch.isnan(ref))


@pytest.mark.parametrize("B,P,matched,with_scale", BC.transform_error_cases())
def test_transform_errors(dev, B, P, matched, with_scale):
    c = BC.transform_error_case(B, P, matched)
    ref = BC.transform_errors_oracle(c, torch.float64, with_scale)
    pts = torch.zeros(1, 3, device=dev)
    got = metrics.compute_transform_errors(pts, pts, c["R_gt"].to(dev), c["t_gt"], c["R_pred"].to(dev), c["t_pred"], c["ppp"], c["anchor"],
                                           matched_part_ids=c["matched"], scale=c["scale"] if with_scale else None, return_per_part=True)
    rm, tm, rot, trans = (x.cpu().double() for x in got)
    skip = (c["ppp"] == 0) | c["anchor"]
    assert float(rot[skip].abs().sum()) == 0.0 and float(trans[skip].abs().sum()) == 0.0       # exactly 0 on anchor and empty parts
    assert _nan_mask_equal(rm, ref[0]) and _nan_mask_equal(tm, ref[1]) and not bool(torch.isnan(rot).any() | torch.isnan(trans).any())
    cls = BC.angle_class_of(c["cls"], ref[2])
    bound = torch.tensor(BC.TE_ROT_BOUND, dtype=torch.float64)[cls]
    e_rot = (rot - ref[2]).abs()
    e_trans = (trans - ref[3]).abs()
    worst = {BC.TE_ANGLES[k]: float(e_rot[~skip & (cls == k)].max()) for k in range(len(BC.TE_ANGLES)) if bool((~skip & (cls == k)).any())}
    ok = ~torch.isnan(ref[0])
    e_rm, e_tm = (rm - ref[0])[ok].abs(), (tm - ref[1])[ok].abs()
    print(f"transform errors B={B} P={P} {matched} scale={with_scale}: rot per angle {worst}, trans {float(e_trans.max()):.2e}, "
          f"means {float(e_rm.max()) if ok.any() else 0:.2e} {float(e_tm.max()) if ok.any() else 0:.2e}")
    floor = lambda r: torch.from_numpy(BC.ulp32(r.numpy()))
    assert bool((e_rot <= torch.maximum(bound, floor(ref[2])))[~skip].all()), worst
    assert bool((e_trans <= torch.maximum(torch.tensor(BC.TE_TRANS_BOUND), floor(ref[3])))[~skip].all()), float(e_trans.max())
    assert bool((e_rm <= torch.maximum(torch.tensor(BC.TE_ROT_MEAN_BOUND), floor(ref[0][ok]))).all())
    assert bool((e_tm <= torch.maximum(torch.tensor(BC.TE_TRANS_MEAN_BOUND), floor(ref[1][ok]))).all())


@pytest.mark.parametrize("B,P,matched,with_scale", BC.transform_error_cases())
def test_transform_errors_direct(dev, B, P, matched, with_scale):
    c = BC.transform_error_case(B, P, matched)
    ref = BC.transform_errors_direct_f64(c, with_scale)
    got = metrics.compute_transform_errors_direct(c["R_gt"].to(dev), c["t_gt"], c["R_pred"].to(dev), c["t_pred"], c["ppp"],
                                                  matched_part_ids=c["matched"], scale=c["scale"] if with_scale else None, return_per_part=True)
    rm, tm, rot, trans = (x.cpu().double() for x in got)
    empty = c["ppp"] == 0
    assert float(rot[empty].abs().sum()) == 0.0 and float(trans[empty].abs().sum()) == 0.0
    assert _nan_mask_equal(rm, ref[0]) and _nan_mask_equal(tm, ref[1]) and not bool(torch.isnan(rot).any() | torch.isnan(trans).any())
    ok = ~torch.isnan(ref[0])
    ulps = []
    for g, r in ((rot, ref[2]), (trans, ref[3]), (rm[ok], ref[0][ok]), (tm[ok], ref[1][ok])):
        u = (g - r).abs() / torch.from_numpy(BC.ulp32(r.numpy()))
        ulps.append(float(u.max()) if u.numel() else 0.0)
    print(f"direct transform errors B={B} P={P} {matched} scale={with_scale}: worst error in fp32 ulp of the reference value (bound "
          f"{BC.TE_DIRECT_ULPS}): rot {ulps[0]:.2f} trans {ulps[1]:.2f} rot mean {ulps[2]:.2f} trans mean {ulps[3]:.2f}")
    assert max(ulps) <= BC.TE_DIRECT_ULPS, ulps


# ---------------------------------------------------------------------------------------------
# 4. generation selection
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", BC.SEL_B)
@pytest.mark.parametrize("G_", BC.SEL_G)
def test_argmin_generation(lib, dev, G_, B):
    """the clouds = NULL form: `best` only"""
    v = BC.selection_values(G_, B)
    vd = v.to(dev)
    for largest in (0, 1):
        best = G.Guarded(4 * B, dev, name="best")
        rc = lib.rap_select_generation(_lib.ptr(vd), G_, B, 1, 0, None, None, None, None, largest, VP(best.ptr), None, None, None, stream(dev))
        assert rc == 0
        best.check()
        ref = torch.argmax(v, dim=0) if largest else torch.argmin(v, dim=0)
        assert torch.equal(best.view(torch.int32, (B,)).cpu().long(), ref), (G_, B, largest)


def _check_gather(c, pick, dev):
    fn = selection.select_generations_by_overlap if pick else selection.select_generations_by_rigidity
    best, cloud, R, t = fn(c["rmse"].to(dev), c["clouds"], c["R"], c["t"], c["cu"])
    ref = torch.argmax(c["rmse"], dim=0) if pick else torch.argmin(c["rmse"], dim=0)
    assert best.dtype == torch.int64 and torch.equal(best.cpu(), ref)
    B = ref.numel()
    tok = torch.repeat_interleave(ref, c["cu"][1:] - c["cu"][:-1])
    assert torch.equal(cloud.cpu(), c["clouds"][tok, torch.arange(tok.numel())])
    assert torch.equal(R.cpu(), c["R"][ref, torch.arange(B)]) and torch.equal(t.cpu(), c["t"][ref, torch.arange(B)])


@pytest.mark.parametrize("pick", [0, 1])
@pytest.mark.parametrize("P", BC.GATHER_P)
def test_gather_generation(dev, P, pick):
    _check_gather(BC.gather_case(P), pick, dev)


def test_gather_generation_past_the_first_block_of_samples(dev):
    """65 samples: the gather of the last one reads a `best` that the second block of argmin_generation_kernel wrote"""
    _check_gather(BC.gather_case(2, counts=tuple([3, 0, 86, 1] * 16 + [90]), G=5), 0, dev)


# ---------------------------------------------------------------------------------------------
# 5. batch tables
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["many", "one_40000", "one_1", "one_16385"])
def test_token_sample(lib, dev, name):
    cu = BC.token_tables()[name]
    B, first, last = cu.numel() - 1, int(cu[0]), int(cu[-1])
    tail = 100
    out = G.Guarded(4 * (last + tail), dev, name="token_sample")                # filled with 0xFF: -1 wherever the kernel did not write
    cu_d = cu.to(dev)
    rc = lib.rap_token_sample(_lib.ptr(cu_d), B, VP(out.ptr), stream(dev))
    assert rc == 0
    out.check()
    got = out.view(torch.int32, (last + tail,)).cpu()
    want = torch.repeat_interleave(torch.arange(B, dtype=torch.int32), (cu[1:] - cu[:-1]).long())
    assert torch.equal(got[first:last], want)
    assert bool((got[:first] == -1).all()) and bool((got[last:] == -1).all())     # entries outside [cu[0], cu[B]) are untouched


@pytest.mark.parametrize("name", list(BC.check_batch_cases()))
def test_check_batch(lib, dev, name):
    ppp, cu, TP, bit = BC.check_batch_cases()[name]
    want = BC.check_batch_bits(ppp, cu, TP)
    flag = torch.full((1,), -1, dtype=torch.int32, device=dev)
    ppp_d, cu_d = torch.tensor(ppp, dtype=torch.int64, device=dev), torch.tensor(cu, dtype=torch.int32, device=dev)
    rc = lib.rap_check_batch(_lib.ptr(ppp_d), _lib.ptr(cu_d), len(ppp), len(ppp[0]), TP, _lib.ptr(flag), stream(dev))
    assert rc == 0
    got = int(flag.item())
    assert got == want and (got & bit) == bit, (name, got, want)
    if name in ("ends_alone", "span_alone", "negative_alone"):
        assert got == bit                                                          # the bits that can be raised alone, alone
