"""The Iceberg sink's own vectors (tests/golden/iceberg_changelog_kats.py, transcribed from crates/etl/src/event.rs and
crates/etl-destinations/src/iceberg/core.rs) against the host model tests/iceberg_changelog.py, which tests/test_gpu_iceberg.py then
holds etlg_batch_iceberg against; plus the constants of include/etlg.h the model restates."""
import os
import re
from types import SimpleNamespace

import pytest

from etl_amd import abi
from tests import iceberg_changelog as IC
from tests.golden import iceberg_changelog_kats as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
USERS = [SimpleNamespace(type_class=abi.TC_I32, type_oid=23), SimpleNamespace(type_class=abi.TC_STRING, type_oid=25)]


@pytest.mark.parametrize("second,commit,want", K.SEQUENCE_NUMBERS)
def test_generate_sequence_number(second, commit, want):
    assert IC.sequence_number(commit, second) == want and len(want) == 33
    assert IC.sequence_number(second, commit) == want[17:] + b"/" + want[:16]       # the commit LSN leads
    assert want == want.lower()


def test_copy_token_is_generate_sequence_number_0_0():
    assert IC.COPY_SEQUENCE == K.SEQUENCE_NUMBERS[0][2] == IC.sequence_number(0, 0)


@pytest.mark.parametrize("kind,want", K.OPERATIONS)
def test_operation_display(kind, want):
    assert IC.OPS[kind] == want and len(want) == 6


@pytest.mark.parametrize("event,row,reason", K.ROW_IMAGES)
def test_row_images(event, row, reason):
    assert IC.choose(event) == (row, reason)
    ev = dict(event, commit_lsn=0x1_0000_00AB, tx_ordinal=7)
    rows, ops, seqs, idx, n_host, first, why = IC.changelog([{"kind": "B"}, ev], 0, USERS)
    if reason:
        assert (rows, ops, seqs, idx, n_host, first, why) == ([], [], [], [], 1, 1, reason)
    else:
        assert rows == [[1, b"alice"]] and ops == [IC.OPS[event["kind"]]] and seqs == [b"00000001000000ab/0000000000000007"]
        assert (idx, n_host, first, why) == ([1], 0, IC.NO_EVENT, 0)
    assert IC.changelog([ev], 1, USERS) == ([], [], [], [], 0, IC.NO_EVENT, 0)                   # another slot's event


def test_refusals_are_counted_and_the_first_is_named_behind_accepted_rows():
    evs = [dict(e, commit_lsn=16, tx_ordinal=k) for k, (e, _, _) in enumerate([K.ROW_IMAGES[0], K.ROW_IMAGES[3], K.ROW_IMAGES[2], K.ROW_IMAGES[1], K.ROW_IMAGES[4]])]
    rows, ops, seqs, idx, n_host, first, why = IC.changelog(evs, 0, USERS)
    assert (ops, idx, n_host, first, why) == ([b"UPDATE", b"DELETE"], [0, 2], 3, 1, IC.KEY_ONLY_DELETE)
    rows, ops, seqs, idx, n_host, first, why = IC.changelog(evs[:1] + [dict(evs[0], kind="I")], 0, USERS, copy=True)
    assert ops == [b"INSERT"] * 2 and seqs == [IC.COPY_SEQUENCE] * 2


def test_descriptions_and_constants():
    assert IC.DESCRIPTIONS == K.DESCRIPTIONS
    hdr = open(os.path.join(ROOT, "include", "etlg.h")).read()
    vals = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define ETLG_ICE_([A-Z_]+) (\d+)u", hdr)}
    assert vals == {"PARTIAL_UPDATE": IC.PARTIAL_UPDATE, "KEY_ONLY_DELETE": IC.KEY_ONLY_DELETE, "DELETE_WITHOUT_OLD_ROW": IC.DELETE_WITHOUT_OLD_ROW}
    assert (abi.ICE_PARTIAL_UPDATE, abi.ICE_KEY_ONLY_DELETE, abi.ICE_DELETE_WITHOUT_OLD_ROW, abi.NO_EVENT) == (1, 2, 3, IC.NO_EVENT)
    import ctypes as C
    assert C.sizeof(abi.ChangelogInfo) == 24
    from etl_amd import native
    assert {"etlg_batch_iceberg", "etlg_columns_changelog_get"} <= set(native.EXPORTS)
