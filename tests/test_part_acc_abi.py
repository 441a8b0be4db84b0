"""CPU: rap_part_acc refuses bad arguments before it touches the device, and rap_part_acc_workspace_bytes is host arithmetic."""
import ctypes

from rap_amd import _lib


def _call(lib, **kw):
    one = ctypes.c_void_p(256)          # a non-NULL sentinel: every call below is refused before a pointer is used
    a = dict(gt=one, pred=one, ppp=one, cu=one, B=2, P=4, TP=100, thr=0.01, acc=one, matched=one, cd=one, ws=one, wsb=1 << 40, stream=None)
    a.update(kw)
    return lib.rap_part_acc(a["gt"], a["pred"], a["ppp"], a["cu"], a["B"], a["P"], a["TP"], a["thr"], a["acc"], a["matched"], a["cd"], a["ws"],
                            a["wsb"], a["stream"])


def test_argument_checks_return_invalid():
    lib = _lib.load()
    N = ctypes.c_void_p(0)
    for name in ("gt", "pred", "ppp", "cu", "acc", "matched"):
        assert _call(lib, **{name: N}) == -1, name
    assert _call(lib, P=0) == -1 and _call(lib, P=-3) == -1 and _call(lib, B=-1) == -1 and _call(lib, TP=-1) == -1
    assert _call(lib, thr=float("nan")) == -1
    assert _call(lib, B=256, P=256) == -1                              # B * P > 65535, the limit of the neighbouring entries
    assert _call(lib, TP=(0x7fffffff // 8) + 1) == -1
    assert _call(lib, B=0) == 0                                        # an empty batch: RAP_OK, nothing launched
    assert _call(lib, B=0, ws=N, wsb=0) == 0


def test_p_257_is_refused():
    lib = _lib.load()
    assert _call(lib, P=257) == -1 and _call(lib, P=256, B=0) == 0
    assert lib.rap_part_acc_workspace_bytes(1000, 2, 257) == 0 and lib.rap_part_acc_workspace_bytes(1000, 2, 256) > 0


def test_short_or_missing_workspace_is_refused_as_by_the_neighbouring_entries():
    """RAP_ERR_WORKSPACE (-2), the code rap_overlap_ratio and rap_chamfer_rmse give for the same defect, after the argument checks"""
    lib = _lib.load()
    need = lib.rap_part_acc_workspace_bytes(100, 2, 4)
    assert _call(lib, ws=ctypes.c_void_p(0)) == -2 and _call(lib, wsb=need - 1) == -2 and _call(lib, wsb=0) == -2
    assert _call(lib, ws=ctypes.c_void_p(0), P=257) == -1              # the argument checks come first


def test_workspace_query_is_monotone_and_of_the_stated_size():
    lib = _lib.load()
    q = lib.rap_part_acc_workspace_bytes
    assert q(-1, 1, 1) == 0 and q(1, -1, 1) == 0 and q(1, 1, -1) == 0
    for B in (1, 3, 32):
        prev = 0
        for TP in (0, 1, 255, 256, 257, 4096, 100000):
            cur = q(TP, B, 6)
            assert cur >= prev and cur > 0, (TP, B)
            prev = cur
        prev = 0
        for P in (1, 2, 31, 32, 33, 64, 65, 255, 256):
            cur = q(5000, B, P)
            assert cur > prev, (P, B)
            prev = cur
    # two planes of TP * P floats + (TP / 256 + B * P + 1) work items of 32 bytes + O(B * P) words, every piece rounded up to 256 bytes
    TP, B, P = 100000, 32, 20
    planes = 2 * TP * P * 4
    rest = (TP // 256 + B * P + 1) * 32 + B * P * 8 + 4 + 2 * B * P * ((P + 31) // 32) * 4
    assert planes + rest <= q(TP, B, P) <= planes + rest + 7 * 256
