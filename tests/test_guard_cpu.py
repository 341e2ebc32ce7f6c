"""The guard-band harness of the containment tests (guard_cases.py) on CPU
tensors, with plain torch writes standing in for a kernel: a clean write
passes, and each planted defect trips the assertion that is there for it.
Also: the table of test_containment_gpu.py covers every device entry of
include/ofdm_lsmrc.h."""
import numpy as np
import pytest

import guard_cases as gc


def _write_all(g):
    import torch
    g.view.copy_(torch.arange(g.view.numel(), dtype=torch.float32).to(g.view.dtype).view(g.shape))


_LAYOUTS = [((3, 7), "complex64"), ((5,), "float32"), ((14,), "int8"), ((1,), "int64"), ((2, 1031, 2), "int16"),
            ((2, 3, 1023), "complex64")]


# an offset below the element size cannot be viewed as that element
@pytest.mark.parametrize("shape,dtype,offset", [(s, d, o) for s, d in _LAYOUTS for o in (0, 4, 8, 16, 256)
                                                if o % np.dtype(d).itemsize == 0])
def test_clean_write_passes_and_layout(shape, dtype, offset):
    g = gc.guarded(shape, dtype, "cpu", offset=offset)
    assert tuple(g.view.shape) == shape and g.view.is_contiguous()
    assert g.view.data_ptr() % (2 * offset if offset else 256) == offset  # exactly that alignment, no more
    row = shape[-1] * np.dtype(dtype).itemsize
    assert g.lo >= max(4096, row) and g.arena.numel() - g.hi >= max(4096, row)
    assert g.unwritten().size == -(-g.nbytes // 4)  # every word still holds the prefill
    g.assert_bands()
    _write_all(g)
    g.assert_bands()
    assert g.unwritten().size == 0


def test_band_and_fill_words_are_quiet_nans():
    for w in (gc.BAND_WORD, gc.FILL_WORD):
        f = np.array([w], np.uint32).view(np.float32)[0]
        assert np.isnan(f) and (w >> 22) & 1 and w & 0x3FFFFF  # quiet bit and a payload
    assert gc.BAND_WORD != gc.FILL_WORD
    g = gc.guarded((4,), "float32", "cpu")
    assert bool(g.view.isnan().all()) and bool(g.arena.view(gc.torch_dtype("float32")).isnan().all())


def test_one_element_before_the_body_trips():
    g = gc.guarded((3, 7), "complex64", "cpu")
    _write_all(g)
    g.arena[g.lo - 8:g.lo].view(gc.torch_dtype("complex64"))[0] = 1.0
    with pytest.raises(AssertionError, match=r"before the body.*\[-8"):
        g.assert_bands()


def test_one_element_after_the_body_trips():
    g = gc.guarded((3, 7), "complex64", "cpu")
    _write_all(g)
    g.arena[g.hi:g.hi + 8].view(gc.torch_dtype("complex64"))[0] = 1.0
    with pytest.raises(AssertionError, match=r"after the body.*\[0"):
        g.assert_bands()


@pytest.mark.parametrize("where", ["first", "just_before", "just_after", "last"])
def test_one_byte_into_either_band_trips(where):
    g = gc.guarded((14,), "int8", "cpu")  # a body that ends inside a word
    _write_all(g)
    i = {"first": 0, "just_before": g.lo - 1, "just_after": g.hi, "last": g.arena.numel() - 1}[where]
    g.arena[i] = int(g.arena[i]) ^ 1
    with pytest.raises(AssertionError, match="1 band byte"):
        g.assert_bands()


def test_a_16_byte_store_over_an_8_byte_row_end_trips():
    """The case the harness is for: the last row of K = C - 1 complex ends 8
    bytes short of a 16-byte line, and a 16-byte store of the last lane spills."""
    g = gc.guarded((2, 3, 1023), "complex64", "cpu")
    _write_all(g)
    g.arena[g.hi - 8:g.hi + 8].view(gc.torch_dtype("float32")).fill_(2.0)
    with pytest.raises(AssertionError, match="8 band byte"):
        g.assert_bands()


def test_an_unwritten_element_trips():
    g = gc.guarded((3, 7), "complex64", "cpu")
    _write_all(g)
    g.view.view(-1)[5] = np.array([gc.FILL_WORD, gc.FILL_WORD], np.uint32).view(np.complex64)[0].item()
    assert g.unwritten().tolist() == [10, 11]
    h = gc.guarded((14,), "int8", "cpu")
    h.view[:12] = 1
    assert h.unwritten().tolist() == [3]  # the ragged tail counts as the last word
    # documented never-written positions are named by element
    m = np.zeros((3, 7), bool)
    m[:, 5:] = True
    assert g.element_words(m).tolist() == [10, 11, 12, 13, 24, 25, 26, 27, 38, 39, 40, 41]


def test_a_modified_input_trips():
    a = (np.arange(21) + 1j).astype(np.complex64).reshape(3, 7)
    g = gc.guarded(a.shape, a.dtype, "cpu", fill=a)
    assert np.array_equal(g.view.numpy(), a)
    g.assert_unmodified()
    g.view[1, 2] += 1e-9j  # below the element's rounding: the bits do not change
    g.assert_unmodified()
    g.view[1, 2] = complex(a[1, 2].real, -a[1, 2].imag)
    with pytest.raises(AssertionError, match="modified"):
        g.assert_unmodified()
    # an output that a later call only reads is frozen where it stands
    o = gc.guarded((5,), "float32", "cpu")
    o.view.fill_(3.0)
    o.freeze().assert_unmodified()
    o.view[4] = -3.0
    with pytest.raises(AssertionError, match=r"modified.*\[19"):
        o.assert_unmodified()
    o.assert_unmodified(mask=np.arange(20) < 16)


def test_poison_prefix():
    iq = np.ones((2, 3, 2, 12), np.complex64)
    p = gc.poison_prefix(iq, 4)
    assert np.array_equal(iq, np.ones_like(iq)) and np.isnan(p[..., :4]).all() and np.array_equal(p[..., 4:], iq[..., 4:])
    assert np.all(p[..., :4].view(np.uint32) == gc.BAND_WORD)
    q = np.zeros((2, 3, 2, 12, 2), np.int16)
    s = gc.poison_prefix(q, 3)
    assert np.all(np.abs(s[..., :3, :]) == 32767) and not s[..., 3:, :].any() and set(np.unique(s)) == {-32767, 0, 32767}
    assert gc.poison_prefix(iq, 0) is not iq and np.array_equal(gc.poison_prefix(iq, 0), iq)


@pytest.mark.parametrize("F,S,R,C", [(2, 4, 3, 1024), (2, 3, 2, 600), (1, 10, 3, 4096), (2, 3, 2, 6)])
def test_guarded_workspace_is_exact(ofdm, F, S, R, C):
    n = ofdm.workspace_bytes(F, S, R, C)
    with gc.guarded_workspace(F, S, R, C, "cpu") as ws:
        assert ws.view.numel() == n == ws.nbytes and ws.view.data_ptr() % 256 == 0
        p = ws.pieces()
        assert p["Hc"] == (0, F * R * C * 8) and p["tickets"][1] <= n
        assert (p["tickets"][1] == n) == (C in (1024, 2048, 4096))  # every other C: the staging buffer follows
        assert all(lo % 256 == 0 for lo, _ in p.values())
        assert int((~ws.ticket_mask()).sum()) == 4096
        ws.assert_bands()
        with gc.guarded_workspace(F, S, R, C, "cpu", offset=256) as w2:
            assert w2.view.numel() == n and w2.view.data_ptr() % 512 == 256
        ws.arena[ws.hi] = 0  # one byte past ofdm_frame_workspace_bytes
        with pytest.raises(AssertionError, match=r"after the body.*\[0\]"):
            ws.assert_bands()


# ------------------------------------------------------------- completeness

def test_table_covers_every_device_entry(ofdm):
    """The entries the table's rows name, with the fixed set of entries that
    touch no caller-supplied device memory, are the ofdm_* functions of the
    header: a new entry point fails here until it has a row."""
    import test_containment_gpu as tc
    header = set(ofdm.header_symbols())
    excluded = set()
    for name in tc.EXCLUDED:
        hit = {s for s in header if s == name or (name.endswith("*") and s.startswith(name[:-1]))}
        assert hit, f"{name} matches no header symbol"
        excluded |= hit
    assert set(tc.EXCLUDED) == set(FIXED_EXCLUSIONS) and all(tc.EXCLUDED.values())
    covered = set()
    for row in tc.TABLE:
        assert row.entries, row.id
        covered |= set(row.entries)
    assert not covered & excluded, sorted(covered & excluded)
    assert covered <= header, sorted(covered - header)
    missing = header - covered - excluded
    assert not missing, f"device entries without a containment row: {sorted(missing)}"
    ids = [row.id for row in tc.TABLE]
    assert len(ids) == len(set(ids))


# the set the exclusion dict may hold, and no other
FIXED_EXCLUSIONS = ["ofdm_version", "ofdm_pilot_rotate", "ofdm_read_pilots", "ofdm_frame_workspace_bytes",
                    "ofdm_device_status*", "ofdm_workspace_release", "ofdm_host_register", "ofdm_host_unregister",
                    "ofdm_pipeline_create*", "ofdm_pipeline_destroy", "ofdm_pipeline_sync", "ofdm_pipeline_set_*",
                    "ofdm_last_error"]
