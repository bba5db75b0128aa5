"""Whole transcripts of the command line on the GPU: return code, stdout, stderr and written files of every command-function
path, byte for byte as recorded before the shared pieces of morna_amd/cli.py were folded (tests/golden/make_cli_golden.py
--transcripts, on an index of tiny_intropolis.tsv).  -m gpu"""
import json
import sys

import pytest

from conftest import GOLDEN

if GOLDEN not in sys.path:
    sys.path.insert(0, GOLDEN)
import make_cli_golden as golden  # noqa: E402

pytestmark = pytest.mark.gpu

with open(golden.TRANSCRIPTS_JSON) as _fh:
    RECORDED = json.load(_fh)


@pytest.fixture(scope="module")
def index_dir(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("cli_transcripts"))
    golden.build_transcript_index(tmp)
    return tmp


def test_the_recorded_transcripts_are_the_case_list():
    stripped = dict((group, [dict((k, v) for k, v in case.items() if k != "result") for case in cases])
                    for group, cases in RECORDED.items())
    assert stripped == json.loads(json.dumps(golden.TRANSCRIPT_GROUPS))


@pytest.mark.parametrize("group", sorted(golden.TRANSCRIPT_GROUPS))
def test_transcripts(index_dir, group):
    for case in RECORDED[group]:
        got = golden.run_transcript(case, index_dir)
        want = case["result"]
        assert got.get("rc") == want.get("rc") and got.get("raises") == want.get("raises"), case["name"]
        assert got == want, case["name"]
