"""ofdm_tx_modulate: the library exports it, the binding declares it, and its
argument checks answer with OFDM_E_ARG before any device work -- no GPU is
touched here (the pointers are never dereferenced)."""
import ctypes

P = ctypes.c_void_p
E_ARG = -1
REFERENCE, RX = 0, 1
PEAK, SCALE = 0, 1


def _call(L, x=4096, ldx=1023, nrows=4, C=1024, cp=16, map=RX, norm=SCALE, scale=1.0, iq=1 << 20, peak=1 << 22):
    rc = L.ofdm_tx_modulate(P(x) if x else None, ldx, nrows, C, cp, map, norm, scale, P(iq) if iq else None,
                            P(peak) if peak else None, None)
    return rc, L.ofdm_last_error()


def test_symbol_exported_and_bound(ofdm):
    L = ofdm.lib()
    assert hasattr(L, "ofdm_tx_modulate")
    assert "ofdm_tx_modulate" in ofdm._SIGS and "ofdm_tx_modulate" in ofdm.header_symbols()
    assert callable(ofdm.tx_modulate)
    assert ofdm.TX_MAPS == {"reference": REFERENCE, "rx": RX} and ofdm.TX_NORMS == {"peak": PEAK, "scale": SCALE}
    hdr = open(ofdm.HEADER_PATH).read()
    for name, v in (("OFDM_TX_MAP_REFERENCE", 0), ("OFDM_TX_MAP_RX", 1), ("OFDM_TX_NORM_PEAK", 0),
                    ("OFDM_TX_NORM_SCALE", 1)):
        assert f"#define {name} {v}\n" in hdr
    assert L.ofdm_version() == 2  # added without a version step


def test_cpuls_tx_api_compiles_and_links(ofdm, tmp_path):
    """modRefSymbol / modOneSymbol of the drop-in cpuLS.hpp, with a non-zero
    prefix macro, compile and link against the library (run on the GPU in
    test_tx_gpu)."""
    import os
    from tx_cases import build_tx_driver
    assert os.path.exists(build_tx_driver(tmp_path, 16))


def test_fft_size(ofdm):
    L = ofdm.lib()
    for C in (1, 0, -4, 8193, 1 << 20):
        rc, err = _call(L, C=C, ldx=1 << 21, cp=0)
        assert rc == E_ARG and b"ofdm_tx_modulate" in err and b"C=" in err, C


def test_prefix_length(ofdm):
    L = ofdm.lib()
    for C, cp in ((1024, -1), (1024, 1025), (64, 65), (2, 3)):
        rc, err = _call(L, C=C, ldx=C, cp=cp)
        assert rc == E_ARG and b"cp_len" in err, (C, cp)


def test_row_pitch_below_k(ofdm):
    L = ofdm.lib()
    for C, ldx in ((1024, 1022), (1024, 0), (1024, -1), (9, 7)):
        rc, err = _call(L, C=C, ldx=ldx, cp=0)
        assert rc == E_ARG and b"ldx" in err, (C, ldx)


def test_unknown_map_or_norm(ofdm):
    L = ofdm.lib()
    for m in (-1, 2, 7):
        rc, err = _call(L, map=m)
        assert rc == E_ARG and b"map" in err
    for n in (-1, 2, 7):
        rc, err = _call(L, norm=n)
        assert rc == E_ARG and b"norm" in err


def test_null_pointers_and_row_count(ofdm):
    L = ofdm.lib()
    rc, err = _call(L, x=0)
    assert rc == E_ARG and b"null" in err
    rc, err = _call(L, iq=0)
    assert rc == E_ARG and b"null" in err
    rc, _ = _call(L, nrows=-1)
    assert rc == E_ARG
    rc, err = _call(L, x=4100)
    assert rc == E_ARG and b"aligned" in err


def test_empty_batch_is_ok(ofdm):
    L = ofdm.lib()
    for C, cp in ((1024, 0), (1024, 1024), (2, 2), (8192, 5), (1536, 0)):
        rc, _ = _call(L, nrows=0, C=C, ldx=C - 1, cp=cp)
        assert rc == 0
    rc, _ = _call(L, nrows=0, x=0, iq=0, peak=0)  # ... with null pointers too
    assert rc == 0
    rc, _ = _call(L, nrows=0, map=3)  # but still not with a bad geometry
    assert rc == E_ARG
