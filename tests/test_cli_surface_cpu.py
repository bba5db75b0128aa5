"""The surface of the command line, pinned before its shared pieces were folded (tests/golden/make_cli_golden.py): what
build_parser() builds, and every refusal that fires before an index is read -- text, type and, where two apply, which one."""
import json
import os
import sys

import pytest

from conftest import GOLDEN

if GOLDEN not in sys.path:
    sys.path.insert(0, GOLDEN)
import make_cli_golden as golden  # noqa: E402

with open(golden.REFUSALS_JSON) as _fh:
    RECORDED = json.load(_fh)


def test_parser_structure_is_the_recorded_one():
    with open(golden.PARSER_JSON) as fh:
        recorded = json.load(fh)
    built = json.loads(json.dumps(golden.parser_structure()))
    assert [s["name"] for s in built] == [s["name"] for s in recorded] and len(built) == 12
    assert sum(len(s["actions"]) for s in built) == 222
    for got, want in zip(built, recorded):
        assert got["help"] == want["help"] and got["exclusive_groups"] == want["exclusive_groups"], got["name"]
        assert got["set_defaults"] == want["set_defaults"], got["name"]
        assert [a["dest"] for a in got["actions"]] == [a["dest"] for a in want["actions"]], got["name"]
        for a, b in zip(got["actions"], want["actions"]):
            assert a == b, (got["name"], a["dest"])
    assert built == recorded


def test_the_recorded_refusals_are_the_case_list():
    assert [dict((k, v) for k, v in r.items() if k != "outcome") for r in RECORDED] == json.loads(json.dumps(golden.REFUSAL_CASES))
    assert all("returns" not in r["outcome"] for r in RECORDED)          # every case is refused


@pytest.mark.parametrize("recorded", RECORDED, ids=[r["name"] for r in RECORDED])
def test_refusal(recorded, tmp_path):
    assert not os.listdir(str(tmp_path))
    assert golden.run_refusal(recorded, str(tmp_path)) == recorded["outcome"]
