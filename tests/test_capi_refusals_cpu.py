"""Every refusal of the frame family of the C ABI, as a whole: return code and
ofdm_last_error() text of each case of capi_refusal_cases.py, byte for byte
what golden/capi_refusals.json recorded.  The checks' order is part of it (the
cases with two faults), and so are the empty-batch no-ops and which entries
consume a raised device status.  Nothing is launched: every case is refused, or
asks for no work, before the first HIP call -- the table holds no other."""
import json
import os

import pytest

import capi_refusal_cases as rc
from helpers import GOLDEN

with open(os.path.join(GOLDEN, "capi_refusals.json")) as _fp:
    RECORDED = json.load(_fp)


def test_table_and_record_cover_each_other():
    assert set(RECORDED) == set(rc.CASES), set(RECORDED) ^ set(rc.CASES)
    assert len(rc.CASES) >= 400
    for cid, want in RECORDED.items():
        rc.check_recordable(cid, want)
    # every entry has cases, and an empty batch or range wherever the entry has one
    for entry in rc.ENTRIES:
        codes = [RECORDED[c]["rc"] for c in rc.CASES if c.startswith(entry + ":")]
        assert rc.ARG in codes, entry
        if entry not in ("ofdm_symbols_demod", "ofdm_frame_export_estimate"):
            assert 0 in codes, entry


def test_binding_knows_every_entry_of_the_table(ofdm):
    sigs = dict(ofdm._all_sigs())
    for entry, (params, _) in rc.ENTRIES.items():
        assert len(params.split()) == len(sigs[entry][1]), entry


@pytest.mark.parametrize("entry", sorted(rc.ENTRIES))
def test_refusals_as_recorded(ofdm, entry):
    L = ofdm.lib()
    L.ofdm_device_status()  # whatever an earlier test left raised
    bad = {}
    for cid in rc.CASES:
        if rc.CASES[cid][0] == entry:
            got = rc.run(L, cid)
            if got != RECORDED[cid]:
                bad[cid] = (got, RECORDED[cid])
    assert not bad, "\n".join(f"{c}:\n   got      {g}\n   recorded {w}" for c, (g, w) in bad.items())
