"""Host self-test of tests/guards.py on CPU tensors: the proof that the guard-band tests CAN fail.  A byte written with a torch op one
past the interior, one before it, or into a row gap makes check() raise with the right offset; an untouched buffer passes.  (No kernel
is ever made to overrun on a GPU to show this.)"""
import re

import pytest
import torch

import guards as G

CPU = torch.device("cpu")


def offsets(excinfo):
    m = re.search(r"first at offset (-?\d+), last at offset (-?\d+)", str(excinfo.value))
    assert m, str(excinfo.value)
    return int(m.group(1)), int(m.group(2))


def test_layout_alignment_fill_and_pad_size():
    for nbytes in (0, 1, 100, 4096, 12345):
        g = G.Guarded(nbytes, CPU, 0xFF)
        assert g.ptr % 256 == 0 and g.interior.numel() == nbytes
        assert g.start >= G.PAD_FLOOR and g.buf.numel() - g.end >= G.PAD_FLOOR
        assert bool((g.interior == 0xFF).all()) and bool((g.buf[:g.start] == 0xA5).all()) and bool((g.buf[g.end:] == 0xA5).all())
        g.check()
        assert g.untouched()
    # derived pad: one 256-row tile at the row pitch, 64 KiB at least
    assert G.pad_bytes(0) == 64 * 1024 and G.pad_bytes(100) == 64 * 1024 and G.pad_bytes(2048) == 256 * 2048 and G.pad_bytes(8192) == 2 << 20
    g = G.Guarded(100 * 2048, CPU, 0xFF, pitch=2048)
    assert g.start >= 256 * 2048 and g.buf.numel() - g.end >= 256 * 2048
    assert torch.isnan(g.view(torch.float32, (100, 512))).all() and torch.isnan(g.view(torch.float16, (100, 1024))).all()
    assert torch.isnan(g.view(torch.bfloat16, (100, 1024))).all() and bool((g.view(torch.int32, (100, 512)) == -1).all())
    assert g.view(torch.float32, (100, 512)).data_ptr() == g.ptr


def test_writes_inside_the_interior_pass():
    g = G.Guarded(1000, CPU, 0xFF)
    g.view(torch.float32, (250,)).fill_(3.0)
    g.check()
    assert not g.untouched()
    s = G.Guarded(10 * 48 * 4, CPU, 0xFF)
    s.strided(torch.float32, 10, 32, 48).fill_(1.0)
    s.check()


def test_a_byte_one_past_the_interior_is_reported_at_offset_0():
    g = G.Guarded(1000, CPU, 0xFF)
    g.buf[g.end] = 0
    with pytest.raises(G.GuardError) as e:
        g.check()
    assert offsets(e) == (0, 0) and "back pad" in str(e.value)
    # two rows of a 512-byte pitch past the end read as offsets 0 .. 1023
    g = G.Guarded(1000, CPU, 0xFF)
    g.buf[g.end:g.end + 1024] = 7
    with pytest.raises(G.GuardError) as e:
        g.check()
    assert offsets(e) == (0, 1023)


def test_a_byte_one_before_the_interior_is_reported():
    g = G.Guarded(1000, CPU, 0xFF)
    g.buf[g.start - 1] = 0xFF
    with pytest.raises(G.GuardError) as e:
        g.check()
    assert offsets(e) == (-1001, -1001) and "front pad" in str(e.value)


def test_a_byte_in_a_row_gap_is_reported():
    rows, cols, ld = 10, 32, 48
    g = G.Guarded(rows * ld * 4, CPU, 0xFF)
    v = g.strided(torch.float32, rows, cols, ld)
    assert v.shape == (rows, cols) and v.stride() == (ld, 1) and v.data_ptr() == g.ptr
    v.fill_(2.0)
    g.check()
    flat = g.view(torch.float32, (rows * ld,))
    assert bool((flat.view(rows, ld)[:, cols:].contiguous().view(torch.uint8) == 0xA5).all())      # the gaps carry the guard byte
    flat[3 * ld + cols] = 2.0           # what a 16-byte store across the end of row 3 does to the first gap element
    with pytest.raises(G.GuardError) as e:
        g.check()
    first, last = offsets(e)
    assert first == (3 * ld + cols) * 4 - rows * ld * 4 and last == first + 3 and "row gap" in str(e.value)
    # the gap after the LAST row counts too
    g = G.Guarded(rows * ld * 4, CPU, 0xFF)
    g.strided(torch.float32, rows, cols, ld)
    g.view(torch.float32, (rows * ld,))[rows * ld - 1] = 0.0
    with pytest.raises(G.GuardError) as e:
        g.check()
    assert offsets(e) == (-4, -1)


def test_input_guards_take_either_pad_content():
    t = torch.arange(12, dtype=torch.float32).reshape(3, 4)
    for byte in (0x00, 0xFF):
        g, v = G.guarded_like(t, CPU, guard=byte)
        assert torch.equal(v, t) and bool((g.buf[:g.start] == byte).all()) and bool((g.buf[g.end:] == byte).all())
        g.check()
        g.buf[g.end + 5] = 1
        with pytest.raises(G.GuardError):
            g.check()


def test_exact_workspaces_replaces_the_name_in_every_module_and_checks_every_buffer(monkeypatch):
    import importlib
    ex = G.exact_workspaces(monkeypatch)
    mods = [importlib.import_module(f"rap_amd.{n}") for n in G.WORKSPACE_MODULES]
    assert all(m.workspace == ex.workspace for m in mods)
    a = mods[0].workspace(CPU, 1000)
    b = mods[-1].workspace(CPU, 4096)
    assert a.numel() == 1000 and b.numel() == 4096 and a.dtype == torch.uint8 and a.data_ptr() % 256 == 0 and len(ex.handed) == 2
    a.fill_(1); b.fill_(2)
    ex.check_all()
    ex.handed[0].buf[ex.handed[0].end] = 0          # one byte past the first workspace's last
    with pytest.raises(G.GuardError) as e:
        ex.check_all()
    assert offsets(e) == (0, 0)
    monkeypatch.undo()
    from rap_amd import flow_model
    assert all(m.workspace is flow_model.workspace for m in mods)
