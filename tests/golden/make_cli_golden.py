#!/usr/bin/env python3
"""Pins the surface of the command line (morna_amd/cli.py) so that its code can be moved without a user or a test seeing it.

    python tests/golden/make_cli_golden.py                      # cli_parser.json and cli_refusals.json (no GPU)
    python tests/golden/make_cli_golden.py --transcripts out.json   # the transcripts (needs the GPU)

The three fixtures were written with the command line as it stood before its shared pieces were folded; they are only
ever regenerated to confirm that the files come out byte for byte the same.

  * cli_parser.json: every subcommand's help, actions, exclusive groups and set_defaults, in order.
  * cli_refusals.json: command lines that are refused before an index is read, with the argparse error line or the exception.
  * cli_transcripts.json: return code, stdout (stderr and written files where named) of command lines on an index of
    tiny_intropolis.tsv.

tests/test_cli_surface_cpu.py and tests/test_gpu_cli_transcripts.py import the case lists and the runners from here.
"""
import argparse
import contextlib
import gzip
import io
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

PARSER_JSON = os.path.join(HERE, "cli_parser.json")
REFUSALS_JSON = os.path.join(HERE, "cli_refusals.json")
TRANSCRIPTS_JSON = os.path.join(HERE, "cli_transcripts.json")

_ACTION_FIELDS = ("option_strings", "dest", "nargs", "const", "default", "choices", "required", "help", "metavar")


def parser_structure():
    """What build_parser() builds, as plain data: per subcommand, in order."""
    from morna_amd import cli
    parser = cli.build_parser()
    sub_action, = [a for a in parser._actions if isinstance(a, argparse._SubParsersAction)]
    helps = dict((c.dest, c.help) for c in sub_action._choices_actions)
    out = []
    for name, sub in sub_action.choices.items():
        actions = []
        for a in sub._actions:
            entry = {"class": type(a).__name__, "type": None if a.type is None else a.type.__name__}
            for field in _ACTION_FIELDS:
                value = getattr(a, field)
                entry[field] = list(value) if isinstance(value, (tuple, list)) else value
            actions.append(dict((k, v) for k, v in entry.items() if v is not None))     # (a field left out is None)
        groups = [{"required": g.required, "members": [a.dest for a in g._group_actions]} for g in sub._mutually_exclusive_groups]
        out.append({"name": name, "help": helps[name], "actions": actions, "exclusive_groups": groups,
                    "set_defaults": dict(sub._defaults)})
    return out


# ---------------------------------------------------------------------------------------------------------- refusals
# files: {path: text}; ["lines", format, n] stands for format % i for i in range(n)
_IDS = {"{tmp}/a.txt": "1\n2\n3\n", "{tmp}/b.txt": "3\n4\n", "{tmp}/g.tsv": "a\t1,2\nb\t3\n", "{tmp}/labels.tsv": "x\t1,2\ny\t3\n"}
_SHARDS = {"{tmp}/idx.shards.mor": ""}
_STORE = {"{tmp}/idx.junc.mor": ""}
_X = ["-x", "{tmp}/idx"]
_J = ["--junction-file", "{tmp}/j.gz"]


def _case(name, argv, files=None, env=None):
    """files: of those offered, the ones the command line names and the ones that stand next to the index."""
    used = dict((path, text) for path, text in (files or {}).items() if path in argv or path.startswith("{tmp}/idx."))
    return {"name": name, "argv": argv, "files": used, "env": dict(env or {})}


def _both(*dicts):
    out = {}
    for d in dicts:
        out.update(d)
    return out


_JUNC = ["junctions"] + _X + _J + ["-sf", "{tmp}/splices"]
_RECALL = ["recall"] + _X + ["--trees", "1,2", "--search-ks", "10,20"]
_HASHING = ["hashing"] + _X + _J + ["--features", "16,index"]
_LABELS = ["labels"] + _X + ["--labels", "{tmp}/labels.tsv"]
_MIXTURE = ["mixture"] + _X + ["--labels", "{tmp}/labels.tsv"]
_PAIRS = ["pairs"] + _X
_CLUSTER = ["cluster"] + _X
_EXPLAIN = ["explain"] + _X + _J
_SUPER = ["supersample"] + _X + _J + ["-o", "{tmp}/pool"]
_WORLD = {"WORLD_SIZE": "2"}

REFUSAL_CASES = [
    # argparse's own
    _case("no-subcommand-flag", ["search"]),
    _case("index-needs-intropolis", ["index"]),
    _case("supersample-needs-one-list", _SUPER),
    _case("supersample-both-lists", _SUPER + ["--sample-ids", "{tmp}/a.txt", "--groups", "{tmp}/g.tsv"], _IDS),
    # search --max-distance
    _case("radius-not-a-number", ["search"] + _X + ["--max-distance", "abc"]),
    _case("radius-without-exact", ["search"] + _X + ["--max-distance", "0.1"]),
    _case("radius-with-rawlist", ["search"] + _X + ["-e", "--max-distance", "0.1", "-rl"]),
    _case("radius-with-backoff", ["search"] + _X + ["-e", "--max-distance", "0.1", "-c", "5"]),
    _case("radius-zero-results", ["search"] + _X + ["-e", "--max-distance", "0.1", "-r", "0"]),
    _case("radius-shards-file", ["search"] + _X + ["-e", "--max-distance", "0.1"], _SHARDS),
    _case("radius-world", ["search"] + _X + ["-e", "--max-distance", "0.1"], env=_WORLD),
    # pairs
    _case("pairs-not-a-number", _PAIRS + ["--max-distance", "abc"]),
    _case("pairs-negative", _PAIRS + ["--max-distance", "-1"]),
    _case("pairs-missing-file", _PAIRS + ["--max-distance", "0.1", "--within", "{tmp}/missing.txt"]),
    _case("pairs-bad-groups", _PAIRS + ["--max-distance", "0.1", "--leave-out-groups", "{tmp}/bad.tsv"], {"{tmp}/bad.tsv": "a 1 2\n"}),
    _case("pairs-within-without", _PAIRS + ["--max-distance", "0.1", "--within", "{tmp}/a.txt", "--without", "{tmp}/b.txt"], _IDS),
    _case("pairs-shards-file", _PAIRS + ["--max-distance", "0.1"], _SHARDS),
    _case("pairs-world", _PAIRS + ["--max-distance", "0.1"], env=_WORLD),
    _case("pairs-order-distance-then-file", _PAIRS + ["--max-distance", "abc", "--within", "{tmp}/missing.txt"]),
    _case("pairs-order-overlap-then-shards", _PAIRS + ["--max-distance", "0.1", "--within", "{tmp}/a.txt", "--without", "{tmp}/b.txt"],
          _both(_IDS, _SHARDS)),
    _case("pairs-order-file-then-world", _PAIRS + ["--max-distance", "0.1", "--without", "{tmp}/missing.txt"], env=_WORLD),
    # cluster
    _case("cluster-exact", _CLUSTER + ["-k", "2", "-e"]),
    _case("cluster-unhashed", _CLUSTER + ["-k", "2", "--unhashed"]),
    _case("cluster-groups", _CLUSTER + ["-k", "2", "--leave-out-groups", "{tmp}/g.tsv"], _IDS),
    _case("cluster-seed-and-init", _CLUSTER + ["--seed", "1", "--init-ids", "{tmp}/a.txt"], _IDS),
    _case("cluster-needs-k", _CLUSTER),
    _case("cluster-iterations", _CLUSTER + ["-k", "2", "--max-iterations", "0"]),
    _case("cluster-missing-file", _CLUSTER + ["-k", "2", "--within", "{tmp}/missing.txt"]),
    _case("cluster-init-twice", _CLUSTER + ["--init-ids", "{tmp}/twice.txt"], {"{tmp}/twice.txt": "1\n2\n1\n"}),
    _case("cluster-k-differs", _CLUSTER + ["-k", "2", "--init-ids", "{tmp}/a.txt"], _IDS),
    _case("cluster-k-zero", _CLUSTER + ["-k", "0"]),
    _case("cluster-k-large", _CLUSTER + ["-k", "4097"]),
    _case("cluster-within-without", _CLUSTER + ["-k", "2", "--within", "{tmp}/a.txt", "--without", "{tmp}/b.txt"], _IDS),
    _case("cluster-shards-file", _CLUSTER + ["-k", "2"], _SHARDS),
    _case("cluster-world", _CLUSTER + ["-k", "2"], env=_WORLD),
    _case("cluster-order-exact-then-k", _CLUSTER + ["-e"]),
    _case("cluster-order-iterations-then-file", _CLUSTER + ["-k", "2", "--max-iterations", "0", "--within", "{tmp}/missing.txt"]),
    _case("cluster-order-k-then-overlap", _CLUSTER + ["-k", "0", "--within", "{tmp}/a.txt", "--without", "{tmp}/b.txt"], _IDS),
    _case("cluster-order-overlap-then-shards", _CLUSTER + ["-k", "2", "--within", "{tmp}/a.txt", "--without", "{tmp}/b.txt"],
          _both(_IDS, _SHARDS)),
    # --downsample
    _case("thin-lost-only-alone", ["recovery"] + _X + ["-q", "1", "--lost-only"]),
    _case("thin-seed-alone", ["search"] + _X + ["-q", "1", "--downsample-seed", "3"]),
    _case("thin-junctions", _JUNC + ["-q", "1", "--downsample", "0.5"]),
    _case("thin-with-intropolis", ["search"] + _X + ["--downsample", "0.5", "--intropolis", "{tmp}/q.gz"]),
    _case("thin-with-sweep", ["recovery"] + _X + ["-q", "1", "--downsample", "0.5", "--results-sweep", "5"]),
    _case("thin-needs-ids", ["search"] + _X + ["--downsample", "0.5"]),
    _case("thin-needs-file", ["search"] + _X + ["-q", "1", "--downsample", "0.5"]),
    _case("thin-recovery-needs-file", ["recovery"] + _X + ["-q", "1", "--downsample", "0.5"]),
    _case("thin-bad-rate", ["search"] + _X + ["-q", "1", "--downsample", "2"] + _J),
    # --within / --without / --leave-out-groups
    _case("restrict-with-rawlist", ["search"] + _X + ["--within", "{tmp}/a.txt", "-rl"], _IDS),
    _case("restrict-missing-file", ["search"] + _X + ["--within", "{tmp}/missing.txt"]),
    _case("restrict-bad-id", ["search"] + _X + ["--without", "{tmp}/bad.txt"], {"{tmp}/bad.txt": "1\nx\n"}),
    _case("restrict-within-without", ["search"] + _X + ["--within", "{tmp}/a.txt", "--without", "{tmp}/b.txt"], _IDS),
    _case("restrict-groups-intropolis", ["search"] + _X + ["--leave-out-groups", "{tmp}/g.tsv", "--intropolis", "{tmp}/q.gz"], _IDS),
    _case("restrict-groups-stream", ["search"] + _X + ["--leave-out-groups", "{tmp}/g.tsv"], _IDS),
    _case("restrict-junctions-overlap", _JUNC + ["--within", "{tmp}/a.txt", "--without", "{tmp}/b.txt"], _IDS),
    _case("restrict-recovery-groups-intropolis",
          ["recovery"] + _X + _J + ["--leave-out-groups", "{tmp}/g.tsv", "--intropolis", "{tmp}/q.gz", "--truth", "{tmp}/t.gz"], _IDS),
    # --supersamples
    _case("pool-recovery", ["recovery"] + _X + ["-q", "1", "--supersamples", "{tmp}/g.tsv"], _IDS),
    _case("pool-junctions", _JUNC + ["--supersamples", "{tmp}/g.tsv"], _IDS),
    _case("pool-needs-file", ["search"] + _X + ["--supersamples", "{tmp}/g.tsv"], _IDS),
    _case("pool-with-query-id", ["search"] + _X + _J + ["--supersamples", "{tmp}/g.tsv", "-q", "1"], _IDS),
    # recovery
    _case("recovery-grid", ["recovery"] + _X + ["-q", "1", "--grid", "x"]),
    _case("recovery-sweep", ["recovery"] + _X + ["-q", "1", "--results-sweep", "x"]),
    _case("recovery-sweep-deeper", ["recovery"] + _X + ["-q", "1", "-r", "5", "--results-sweep", "2,10"]),
    _case("recovery-distances", ["recovery"] + _X + ["-q", "1", "-d"]),
    _case("recovery-unhashed", ["recovery"] + _X + ["-q", "1", "--unhashed"]),
    _case("recovery-needs-query", ["recovery"] + _X),
    _case("recovery-needs-truth", ["recovery"] + _X + ["--intropolis", "{tmp}/q.gz"]),
    _case("recovery-truth-alone", ["recovery"] + _X + ["-q", "1", "--truth", "{tmp}/t.gz"]),
    _case("recovery-order-thin-then-grid", ["recovery"] + _X + ["-q", "1", "--lost-only", "--grid", "x"]),
    _case("recovery-order-grid-then-batch", ["recovery"] + _X + ["--grid", "x", "--query-ids", "1,b"]),
    _case("recovery-order-flags-then-batch", ["recovery"] + _X + ["-m", "--query-ids", "1,b"]),
    _case("recovery-order-batch-then-restrict", ["recovery"] + _X + ["--query-ids", "1,b", "--within", "{tmp}/missing.txt"]),
    _case("recovery-order-pool-then-grid", ["recovery"] + _X + ["-q", "1", "--supersamples", "{tmp}/g.tsv", "--grid", "x"], _IDS),
    # search --use-trees
    _case("trees-zero", ["search"] + _X + ["--use-trees", "0"]),
    _case("trees-exact", ["search"] + _X + ["--use-trees", "2", "-e"]),
    _case("trees-groups", ["search"] + _X + ["-q", "1", "--use-trees", "2", "--leave-out-groups", "{tmp}/g.tsv"], _IDS),
    # recall
    _case("recall-no-source", _RECALL),
    _case("recall-two-sources", _RECALL + ["-q", "1", "--sample", "3"]),
    _case("recall-bad-ids", _RECALL + ["--query-ids", "1,b"]),
    _case("recall-seed-alone", _RECALL + ["-q", "1", "--sample-seed", "1"]),
    _case("recall-sample-zero", _RECALL + ["--sample", "0"]),
    _case("recall-results", _RECALL + ["-q", "1", "-r", "257"]),
    _case("recall-lists", ["recall"] + _X + ["-q", "1", "--trees", "2,1", "--search-ks", "10"]),
    _case("recall-world", _RECALL + ["-q", "1"], env=_WORLD),
    _case("recall-shards-file", _RECALL + ["-q", "1"], _SHARDS),
    _case("recall-order-source-then-ids", _RECALL + ["--query-ids", "1,b", "--sample", "3"]),
    _case("recall-order-ids-then-results", _RECALL + ["--query-ids", "1,b", "-r", "0"]),
    _case("recall-order-seed-then-lists", ["recall"] + _X + ["-q", "1", "--sample-seed", "1", "--trees", "2,1", "--search-ks", "10"]),
    _case("recall-order-lists-then-world", ["recall"] + _X + ["-q", "1", "--trees", "1", "--search-ks", "20,10"], env=_WORLD),
    _case("recall-order-world-then-shards", _RECALL + ["-q", "1"], _SHARDS, _WORLD),
    # hashing
    _case("hashing-exact", _HASHING + ["-q", "1", "-e"]),
    _case("hashing-within", _HASHING + ["-q", "1", "--within", "{tmp}/a.txt"], _IDS),
    _case("hashing-intropolis", _HASHING + ["--intropolis", "{tmp}/q.gz"]),
    _case("hashing-no-source", _HASHING),
    _case("hashing-two-sources", _HASHING + ["-q", "1", "--query-ids", "1,2"]),
    _case("hashing-bad-ids", _HASHING + ["--query-ids", "1,b"]),
    _case("hashing-seed-alone", _HASHING + ["-q", "1", "--sample-seed", "1"]),
    _case("hashing-sample-zero", _HASHING + ["--sample", "0"]),
    _case("hashing-results", _HASHING + ["-q", "1", "-r", "0"]),
    _case("hashing-search-k-alone", _HASHING + ["-q", "1", "--search-k", "50"]),
    _case("hashing-trees-zero", _HASHING + ["-q", "1", "--n-trees", "0"]),
    _case("hashing-search-k-zero", _HASHING + ["-q", "1", "--n-trees", "2", "--search-k", "0"]),
    _case("hashing-features", ["hashing"] + _X + _J + ["-q", "1", "--features", "64,16"]),
    _case("hashing-features-index-twice", ["hashing"] + _X + _J + ["-q", "1", "--features", "index,index"]),
    _case("hashing-world", _HASHING + ["-q", "1"], env=_WORLD),
    _case("hashing-shards-file", _HASHING + ["-q", "1"], _SHARDS),
    _case("hashing-no-store", _HASHING + ["-q", "1"]),
    _case("hashing-no-weights", _HASHING + ["-q", "1"], _STORE),
    _case("hashing-order-refused-then-source", _HASHING + ["--unhashed"]),
    _case("hashing-order-ids-then-features", ["hashing"] + _X + _J + ["--query-ids", "1,b", "--features", "64,16"]),
    _case("hashing-order-features-then-world", ["hashing"] + _X + _J + ["-q", "1", "--features", "64,16"], env=_WORLD),
    _case("hashing-order-shards-then-store", _HASHING + ["-q", "1"], _SHARDS),
    # labels
    _case("labels-two-sources", _LABELS + ["-q", "1", "--all"], _IDS),
    _case("labels-format", _LABELS + ["-f", "bam"], _IDS),
    _case("labels-bad-ids", _LABELS + ["--query-ids", "1,b"], _IDS),
    _case("labels-seed-alone", _LABELS + ["--all", "--sample-seed", "1"], _IDS),
    _case("labels-sample-zero", _LABELS + ["--sample", "0"], _IDS),
    _case("labels-top", _LABELS + ["--all", "--top", "0"], _IDS),
    _case("labels-matrix-stream", _LABELS + ["--matrix"], _IDS),
    _case("labels-matrix-intropolis", _LABELS + ["--matrix", "--intropolis", "{tmp}/q.gz"], _IDS),
    _case("labels-groups-stream", _LABELS + ["--leave-out-groups", "{tmp}/g.tsv"], _IDS),
    _case("labels-missing-file", ["labels"] + _X + ["--labels", "{tmp}/missing.tsv", "--all"]),
    _case("labels-no-label", ["labels"] + _X + ["--labels", "{tmp}/empty.tsv", "--all"], {"{tmp}/empty.tsv": ""}),
    _case("labels-too-many", ["labels"] + _X + ["--labels", "{tmp}/many.tsv", "--all"], {"{tmp}/many.tsv": ["lines", "l%d\t%d\n", 4097]}),
    _case("labels-within-without", _LABELS + ["--all", "--within", "{tmp}/a.txt", "--without", "{tmp}/b.txt"], _IDS),
    _case("labels-world", _LABELS + ["--all"], _IDS, _WORLD),
    _case("labels-shards-file", _LABELS + ["--all"], _both(_IDS, _SHARDS)),
    _case("labels-order-source-then-format", _LABELS + ["-q", "1", "--all", "-f", "bam"], _IDS),
    _case("labels-order-top-then-file", ["labels"] + _X + ["--labels", "{tmp}/missing.tsv", "--all", "--top", "0"]),
    _case("labels-order-matrix-then-overlap", _LABELS + ["--matrix", "--within", "{tmp}/a.txt", "--without", "{tmp}/b.txt"], _IDS),
    _case("labels-order-overlap-then-world", _LABELS + ["--all", "--within", "{tmp}/a.txt", "--without", "{tmp}/b.txt"], _IDS, _WORLD),
    # mixture
    _case("mixture-exact", _MIXTURE + ["--all", "-e"], _IDS),
    _case("mixture-pool", _MIXTURE + ["--supersamples", "{tmp}/g.tsv"], _IDS),
    _case("mixture-min-share", _MIXTURE + ["--all", "--min-share", "1.5"], _IDS),
    _case("mixture-tolerance", _MIXTURE + ["--all", "--tolerance", "-1"], _IDS),
    _case("mixture-tolerance-nan", _MIXTURE + ["--all", "--tolerance", "nan"], _IDS),
    _case("mixture-sweeps", _MIXTURE + ["--all", "--max-sweeps", "0"], _IDS),
    _case("mixture-two-sources", _MIXTURE + ["-q", "1", "--all"], _IDS),
    _case("mixture-too-many", ["mixture"] + _X + ["--labels", "{tmp}/many.tsv", "--all"], {"{tmp}/many.tsv": ["lines", "l%d\t%d\n", 129]}),
    _case("mixture-world", _MIXTURE + ["--all"], _IDS, _WORLD),
    _case("mixture-shards-file", _MIXTURE + ["--all"], _both(_IDS, _SHARDS)),
    _case("mixture-order-refused-then-source", _MIXTURE + ["-q", "1", "--all", "--unhashed"], _IDS),
    _case("mixture-order-sweeps-then-format", _MIXTURE + ["--max-sweeps", "0", "-f", "bam"], _IDS),
    _case("mixture-order-share-then-file", ["mixture"] + _X + ["--labels", "{tmp}/missing.tsv", "--all", "--min-share", "-0.5"]),
    _case("mixture-order-many-then-world", ["mixture"] + _X + ["--labels", "{tmp}/many.tsv", "--all"],
          {"{tmp}/many.tsv": ["lines", "l%d\t%d\n", 129]}, _WORLD),
    _case("mixture-order-overlap-then-many",
          ["mixture"] + _X + ["--labels", "{tmp}/many.tsv", "--all", "--within", "{tmp}/a.txt", "--without", "{tmp}/b.txt"],
          _both(_IDS, {"{tmp}/many.tsv": ["lines", "l%d\t%d\n", 129]})),
    # explain
    _case("explain-two-sources", _EXPLAIN + ["-q", "1", "--sample", "2"]),
    _case("explain-format", _EXPLAIN + ["-f", "bam"]),
    _case("explain-bad-ids", _EXPLAIN + ["--query-ids", "1,b"]),
    _case("explain-seed-alone", _EXPLAIN + ["-q", "1", "--sample-seed", "1"]),
    _case("explain-sample-zero", _EXPLAIN + ["--sample", "0"]),
    _case("explain-top", _EXPLAIN + ["-q", "1", "--top", "65"]),
    _case("explain-results", _EXPLAIN + ["-q", "1", "-r", "1025"]),
    _case("explain-against-results", _EXPLAIN + ["-q", "1", "--against", "2", "-r", "5"]),
    _case("explain-against-within", _EXPLAIN + ["-q", "1", "--against", "2", "--within", "{tmp}/a.txt"], _IDS),
    _case("explain-against-bad-ids", _EXPLAIN + ["-q", "1", "--against", "2,b"]),
    _case("explain-against-too-many", _EXPLAIN + ["-q", "1", "--against", ",".join(["1"] * 1025)]),
    _case("explain-unhashed-exact", _EXPLAIN + ["-q", "1", "--unhashed", "-e"]),
    _case("explain-missing-file", _EXPLAIN + ["-q", "1", "--without", "{tmp}/missing.txt"]),
    _case("explain-within-without", _EXPLAIN + ["-q", "1", "--within", "{tmp}/a.txt", "--without", "{tmp}/b.txt"], _IDS),
    _case("explain-shards-file", _EXPLAIN + ["-q", "1"], _SHARDS),
    _case("explain-world", _EXPLAIN + ["-q", "1"], env=_WORLD),
    _case("explain-no-store", _EXPLAIN + ["-q", "1"]),
    _case("explain-no-weights", _EXPLAIN + ["-q", "1"], _STORE),
    _case("explain-order-source-then-top", _EXPLAIN + ["-q", "1", "--sample", "2", "--top", "0"]),
    _case("explain-order-results-then-against", _EXPLAIN + ["-q", "1", "-r", "0", "--against", "2"]),
    _case("explain-order-against-then-overlap", _EXPLAIN + ["-q", "1", "--against", "2,b", "--within", "{tmp}/missing.txt"]),
    _case("explain-order-overlap-then-shards", _EXPLAIN + ["-q", "1", "--within", "{tmp}/a.txt", "--without", "{tmp}/b.txt"],
          _both(_IDS, _SHARDS)),
    _case("explain-order-shards-then-store", _EXPLAIN + ["-q", "1"], _SHARDS),
    # --intropolis / --query-ids of search, junctions, recovery
    _case("batch-both", ["search"] + _X + ["--intropolis", "{tmp}/q.gz", "--query-ids", "1,2"]),
    _case("batch-with-query-id", ["search"] + _X + ["--query-ids", "1,2", "-q", "1"]),
    _case("batch-intropolis-backoff", ["search"] + _X + ["--intropolis", "{tmp}/q.gz", "-c", "5"]),
    _case("batch-bad-ids", ["search"] + _X + ["--query-ids", "1,b"]),
    # --unhashed
    _case("unhashed-junctions", _JUNC + ["--unhashed"]),
    _case("unhashed-exact", ["search"] + _X + ["--unhashed", "-e"]),
    _case("unhashed-search-k", ["search"] + _X + ["--unhashed", "-q", "1", "--search-k", "50"]),
    _case("unhashed-stream-needs-file", ["search"] + _X + ["--unhashed"]),
    _case("unhashed-intropolis-needs-file", ["search"] + _X + ["--unhashed", "--intropolis", "{tmp}/q.gz"]),
    # junctions
    _case("junctions-filter", _JUNC + ["--junction-filter", "x"]),
    _case("junctions-rawlist", _JUNC + ["-rl"]),
    _case("junctions-order-thin-then-filter", _JUNC + ["--downsample-seed", "3", "--junction-filter", "x"]),
    _case("junctions-order-batch-then-unhashed", _JUNC + ["--query-ids", "1,b", "--unhashed"]),
    _case("junctions-order-unhashed-then-filter", _JUNC + ["--unhashed", "--junction-filter", "x"]),
    _case("junctions-order-filter-then-restrict", _JUNC + ["--junction-filter", "x", "--within", "{tmp}/missing.txt"]),
    _case("junctions-order-rawlist-then-restrict", _JUNC + ["-rl", "--within", "{tmp}/a.txt"], _IDS),
    # search: two refusals of different checks at once
    _case("search-order-thin-then-pool", ["search"] + _X + ["--downsample-seed", "3", "--supersamples", "{tmp}/g.tsv"], _IDS),
    _case("search-order-pool-then-batch", ["search"] + _X + ["--supersamples", "{tmp}/g.tsv", "--query-ids", "1,b"], _IDS),
    _case("search-order-batch-then-unhashed", ["search"] + _X + ["--query-ids", "1,b", "--unhashed", "-e"]),
    _case("search-order-unhashed-then-restrict", ["search"] + _X + ["--unhashed", "--within", "{tmp}/missing.txt"]),
    _case("search-order-restrict-then-trees", ["search"] + _X + ["--within", "{tmp}/missing.txt", "--use-trees", "2"]),
    _case("search-order-trees-then-radius", ["search"] + _X + ["--use-trees", "0", "--max-distance", "abc"]),
    _case("search-order-trees-then-radius-flags", ["search"] + _X + ["--use-trees", "2", "-e", "--max-distance", "0.1"]),
    # after the parser, before an index is opened
    _case("main-world-junctions", _JUNC + ["-q", "1"], _SHARDS, _WORLD),
    _case("main-world-recovery", ["recovery"] + _X + ["-q", "1"], _SHARDS, _WORLD),
    _case("main-world-unhashed", ["search"] + _X + ["-q", "1", "--unhashed"], _SHARDS, _WORLD),
    _case("main-world-pool", ["search"] + _X + _J + ["--supersamples", "{tmp}/g.tsv"], _both(_IDS, _SHARDS), _WORLD),
    _case("main-world-thin", ["search"] + _X + _J + ["-q", "1", "--downsample", "0.5"], _SHARDS, _WORLD),
    _case("main-world-trees", ["search"] + _X + ["-q", "1", "--use-trees", "2"], _SHARDS, _WORLD),
    _case("main-junctions-results", _JUNC + ["-q", "1", "-r", "65"]),
    _case("main-recovery-results", ["recovery"] + _X + ["-q", "1", "-r", "65"]),
    _case("main-junctions-no-store", _JUNC + ["-q", "1"]),
    _case("main-recovery-no-store", ["recovery"] + _X + ["-q", "1"]),
    _case("main-thin-no-store", ["search"] + _X + _J + ["-q", "1", "--downsample", "0.5"]),
    _case("main-order-world-then-results", _JUNC + ["-q", "1", "-r", "65"], _SHARDS, _WORLD),
    _case("main-order-results-then-store", ["recovery"] + _X + ["-q", "1", "-r", "65"]),
    _case("supersample-missing-ids", _SUPER + ["--sample-ids", "{tmp}/missing.txt"]),
    _case("supersample-bad-groups", _SUPER + ["--groups", "{tmp}/bad.tsv"], {"{tmp}/bad.tsv": "a 1 2\n"}),
    _case("supersample-no-store", _SUPER + ["--groups", "{tmp}/g.tsv"], _IDS),
    _case("supersample-order-file-then-store", _SUPER + ["--sample-ids", "{tmp}/bad.txt"], {"{tmp}/bad.txt": "1\nx\n"}),
]


def _file_text(spec):
    if isinstance(spec, list):
        kind, fmt, n = spec
        assert kind == "lines"
        return "".join(fmt % (i, i) for i in range(n))
    return spec


def run_refusal(case, tmp):
    """One refusal case in the directory tmp (fresh): {"exit": code, "error": the "error: ..." line} or {"raises": type,
    "text": str}, with tmp written as {tmp}."""
    from morna_amd import cli
    for path, spec in case["files"].items():
        with open(path.replace("{tmp}", tmp), "w") as fh:
            fh.write(_file_text(spec))
    saved = os.environ.pop("WORLD_SIZE", None)
    os.environ.update(case["env"])
    err = io.StringIO()
    try:
        with contextlib.redirect_stderr(err), contextlib.redirect_stdout(io.StringIO()):
            rc = cli.main([a.replace("{tmp}", tmp) for a in case["argv"]], stdin=io.StringIO(""), stdout=io.StringIO())
        outcome = {"returns": rc}
    except SystemExit as e:
        last = err.getvalue().rstrip("\n").split("\n")[-1]
        outcome = {"exit": e.code, "error": last[last.index("error: "):]}
    except Exception as e:                                     # noqa: BLE001  (the type is what is recorded)
        outcome = {"raises": type(e).__name__, "text": str(e)}
    finally:
        for name in case["env"]:
            os.environ.pop(name, None)
        if saved is not None:
            os.environ["WORLD_SIZE"] = saved
    return json.loads(json.dumps(outcome).replace(tmp, "{tmp}"))


# -------------------------------------------------------------------------------------------------------- transcripts
_I = ["-x", "{tmp}/idx"]
_JF = ["--junction-file", "{tmp}/tiny.tsv.gz"]
_Q = "{tmp}/queries.gz"
_RAW = "chr1\t14830\t14929\t3\nchr1\t14830\t14969\t5\nchr1\t14830\t14929\t1\nchrUn\t1\t2\t8\n"
_SAM = "".join("r\t0\tchr1\t%d\t255\t10M%dN10M\t*\t0\t0\t*\t*\n" % (s - 10, e - s + 1)
               for s, e in ((14830, 14929), (14830, 14969), (14830, 14969), (15039, 15795), (14830, 14969)))
_WITHIN = [1, 3, 5, 7, 12, 13, 18, 20, 24, 28, 33, 36, 43, 44, 51, 52, 53, 54, 56, 57, 58, 63, 65, 66]


def _t(name, argv, stdin=None, stderr=False, outputs=()):
    return {"name": name, "argv": argv, "stdin": stdin, "stderr": stderr, "outputs": list(outputs)}


_S5 = ["search"] + _I + ["-d", "-r", "5"]
_RADIUS = ["-e", "--max-distance", "0.05"]
_THIN = ["--query-ids", "12,58", "--downsample", "0.5,0"] + _JF
_LAB = ["--labels", "{tmp}/labels.tsv"]
_REC = ["recovery"] + _I + ["--query-ids", "12,33,58", "-r", "5", "--grid", "0,.5:1,5"]

TRANSCRIPT_GROUPS = {
    "search": [
        _t("stream", _S5 + ["-f", "raw"], _RAW),
        _t("stream-exact-meta", _S5 + ["-f", "raw", "-e", "-m"], _RAW),
        _t("stream-sam-backoff", ["search"] + _I + ["-r", "5", "-c", "1", "-ch", "1"], _SAM),
        _t("stream-rawlist", ["search"] + _I + ["-f", "raw", "-rl"], _RAW),
        _t("query-id", _S5 + ["-q", "58"]),
        _t("query-id-exact-meta", _S5 + ["-q", "58", "-e", "-m"]),
        _t("query-ids", _S5 + ["--query-ids", "12,33,58", "-m"]),
        _t("query-ids-exact", ["search"] + _I + ["-r", "5", "--query-ids", "12,33", "-e"]),
        _t("intropolis", _S5 + ["--intropolis", _Q]),
        _t("intropolis-exact", _S5 + ["--intropolis", _Q, "-e", "-m"]),
        _t("use-trees-query-ids", _S5 + ["--query-ids", "12,33", "--use-trees", "2", "--search-k", "50"]),
        _t("use-trees-query-id", _S5 + ["-q", "58", "--use-trees", "2"]),
        _t("use-trees-intropolis", _S5 + ["--intropolis", _Q, "--use-trees", "2"]),
        _t("use-trees-stream", _S5 + ["-f", "raw", "--use-trees", "2"], _RAW),
    ],
    "search_radius_unhashed": [
        _t("radius-query-ids", ["search"] + _I + _RADIUS + ["--query-ids", "12,33", "-d", "-r", "6"]),
        _t("radius-query-id", ["search"] + _I + _RADIUS + ["-q", "58", "-d", "-r", "4", "-m"]),
        _t("radius-intropolis", ["search"] + _I + _RADIUS + ["--intropolis", _Q, "-d", "-r", "4"]),
        _t("radius-stream", ["search"] + _I + _RADIUS + ["-f", "raw", "-d", "-r", "4"], _RAW),
        _t("radius-within-groups", ["search"] + _I + _RADIUS + ["--query-ids", "12,33", "-d", "--within", "{tmp}/within.txt",
                                                                 "--leave-out-groups", "{tmp}/groups.tsv"], stderr=True),
        _t("unhashed-query-ids", _S5 + ["--unhashed", "--query-ids", "12,58", "-m"]),
        _t("unhashed-query-id", _S5 + ["--unhashed", "-q", "33"]),
        _t("unhashed-intropolis", _S5 + ["--unhashed", "--intropolis", _Q] + _JF),
        _t("unhashed-stream", _S5 + ["--unhashed", "-f", "raw"] + _JF, _RAW),
        _t("unhashed-within", _S5 + ["--unhashed", "-q", "33", "--within", "{tmp}/within.txt"], stderr=True),
    ],
    "search_restricted": [
        _t("within-query-id", _S5 + ["-q", "58", "--within", "{tmp}/within.txt"], stderr=True),
        _t("within-query-ids-exact", _S5 + ["--query-ids", "12,33", "-e", "--within", "{tmp}/within.txt"], stderr=True),
        _t("within-intropolis-exact", _S5 + ["--intropolis", _Q, "-e", "--within", "{tmp}/within.txt"], stderr=True),
        _t("within-intropolis", _S5 + ["--intropolis", _Q, "--within", "{tmp}/within.txt"], stderr=True),
        _t("without-stream", _S5 + ["-f", "raw", "--without", "{tmp}/within.txt"], _RAW, stderr=True),
        _t("without-stream-exact", _S5 + ["-f", "raw", "-e", "--without", "{tmp}/within.txt"], _RAW, stderr=True),
        _t("groups-query-ids", _S5 + ["--query-ids", "12,33,1", "--leave-out-groups", "{tmp}/groups.tsv"], stderr=True),
        _t("groups-query-id-exact", _S5 + ["-q", "12", "-e", "--leave-out-groups", "{tmp}/groups.tsv"], stderr=True),
    ],
    "search_pooled_thinned": [
        _t("pool", _S5 + ["--supersamples", "{tmp}/pools.tsv"] + _JF),
        _t("pool-exact-within", _S5 + ["--supersamples", "{tmp}/pools.tsv", "-e", "--within", "{tmp}/within.txt", "-m"] + _JF,
           stderr=True),
        _t("pool-unhashed", _S5 + ["--supersamples", "{tmp}/pools.tsv", "--unhashed"] + _JF),
        _t("pool-radius", ["search"] + _I + _RADIUS + ["--supersamples", "{tmp}/pools.tsv", "-d", "-r", "4"] + _JF),
        _t("pool-use-trees", _S5 + ["--supersamples", "{tmp}/pools.tsv", "--use-trees", "2"] + _JF),
        _t("thin", _S5 + _THIN, stderr=True),
        _t("thin-exact-keeps-none", _S5 + _THIN + ["-e", "-m"], stderr=True),
        _t("thin-unhashed", _S5 + ["--query-ids", "12,58", "--downsample", "0.5,0", "--unhashed"], stderr=True),
        _t("thin-radius", ["search"] + _I + _RADIUS + ["-q", "58", "--downsample", "0.9", "-d", "-r", "4"] + _JF, stderr=True),
        _t("thin-groups", _S5 + ["--query-ids", "12,33", "--downsample", "0.9", "--leave-out-groups", "{tmp}/groups.tsv"] + _JF,
           stderr=True),
        _t("thin-groups-exact", _S5 + ["--query-ids", "12,33", "--downsample", "0.9", "-e", "--leave-out-groups",
                                       "{tmp}/groups.tsv"] + _JF, stderr=True),
        _t("thin-use-trees", _S5 + ["-q", "58", "--downsample", "0.9", "--use-trees", "2"] + _JF, stderr=True),
    ],
    "junctions_recovery_supersample": [
        _t("junctions-pass1", ["junctions"] + _I + _JF + ["-p1", "{tmp}/pass1.sam", "-sf", "{tmp}/splice", "-r", "5"], stderr=True,
           outputs=["{tmp}/splice"]),
        _t("junctions-query-id", ["junctions"] + _I + _JF + ["-q", "58", "-sf", "{tmp}/splice1", "-r", "5", "-d"], stderr=True,
           outputs=["{tmp}/splice1"]),
        _t("junctions-query-ids", ["junctions"] + _I + _JF + ["--query-ids", "12,33", "-sf", "{tmp}/spliceb", "-r", "5", "-e",
                                                              "--junction-filter", ".5,3"], stderr=True,
           outputs=["{tmp}/spliceb.12", "{tmp}/spliceb.33"]),
        _t("junctions-intropolis-within", ["junctions"] + _I + _JF + ["--intropolis", _Q, "-sf", "{tmp}/splicei", "-r", "5", "--within",
                                                                      "{tmp}/within.txt"], stderr=True,
           outputs=["{tmp}/splicei.70000", "{tmp}/splicei.70001"]),
        _t("recovery", _REC),
        _t("recovery-exact-query-id", ["recovery"] + _I + ["-q", "58", "-r", "5", "-e"]),
        _t("recovery-sweep", _REC + ["--results-sweep", "2,5", "--summary-only"]),
        _t("recovery-thin-lost-only", _REC + ["--downsample", "0.5,0.1", "--lost-only"] + _JF, stderr=True),
        _t("recovery-thin-exact-keeps-none", _REC + ["--downsample", "0", "-e", "--summary-only"] + _JF, stderr=True),
        _t("recovery-groups", _REC + ["--leave-out-groups", "{tmp}/groups.tsv"], stderr=True),
        _t("recovery-intropolis-truth", ["recovery"] + _I + _JF + ["--intropolis", _Q, "--truth", "{tmp}/truth.gz", "-r", "5", "--grid",
                                                                   "0,.5:1,5"], stderr=True),
        _t("supersample-groups", ["supersample"] + _I + _JF + ["--groups", "{tmp}/pools.tsv", "-o", "{tmp}/pool"],
           outputs=["{tmp}/pool.first", "{tmp}/pool.second"]),
        _t("supersample-ids", ["supersample"] + _I + _JF + ["--sample-ids", "{tmp}/within.txt", "-o", "{tmp}/pooled"],
           outputs=["{tmp}/pooled"]),
    ],
    "recall_hashing": [
        _t("recall-sample", ["recall"] + _I + ["--sample", "5", "-r", "5", "--trees", "1,2,all", "--search-ks", "10,100"]),
        _t("recall-query-ids", ["recall"] + _I + ["--query-ids", "12,58", "-r", "5", "--trees", "2,4", "--search-ks", "50", "--summary-only"]),
        _t("recall-query-id", ["recall"] + _I + ["-q", "33", "-r", "3", "--trees", "all", "--search-ks", "50"]),
        _t("recall-intropolis", ["recall"] + _I + ["--intropolis", _Q, "-r", "5", "--trees", "1,4", "--search-ks", "20,40"]),
        _t("hashing-sample", ["hashing"] + _I + _JF + ["--sample", "4", "--sample-seed", "7", "-r", "5", "--features", "16,64,index"]),
        _t("hashing-query-ids-forest", ["hashing"] + _I + _JF + ["--query-ids", "12,58", "-r", "5", "--features", "32,index", "--n-trees",
                                                                 "2", "--search-k", "50", "--summary-only"]),
        _t("hashing-query-id", ["hashing"] + _I + _JF + ["-q", "33", "-r", "5", "--features", "index"]),
    ],
    "labels_mixture": [
        _t("labels-all-matrix", ["labels"] + _I + _LAB + ["--all", "--matrix", "--summary-only"]),
        _t("labels-intropolis", ["labels"] + _I + _LAB + ["--intropolis", _Q, "--top", "2"]),
        _t("labels-stream", ["labels"] + _I + _LAB + ["-f", "raw"], _RAW),
        _t("labels-query-ids-restricted", ["labels"] + _I + _LAB + ["--query-ids", "12,33,1", "--within", "{tmp}/within.txt",
                                                                    "--leave-out-groups", "{tmp}/groups.tsv", "--matrix"], stderr=True),
        _t("labels-sample", ["labels"] + _I + _LAB + ["--sample", "5", "--sample-seed", "3", "--top", "1"]),
        _t("labels-query-id", ["labels"] + _I + _LAB + ["-q", "58"]),
        _t("mixture-all-matrix", ["mixture"] + _I + _LAB + ["--all", "--matrix", "--summary-only"]),
        _t("mixture-intropolis", ["mixture"] + _I + _LAB + ["--intropolis", _Q, "--top", "2"]),
        _t("mixture-stream", ["mixture"] + _I + _LAB + ["-f", "raw", "--min-share", "0.2"], _RAW),
        _t("mixture-query-ids-restricted", ["mixture"] + _I + _LAB + ["--query-ids", "12,33,1", "--without", "{tmp}/without.txt",
                                                                      "--matrix"], stderr=True),
        _t("mixture-sample", ["mixture"] + _I + _LAB + ["--sample", "5", "--sample-seed", "3", "--top", "1"]),
    ],
    "pairs_cluster": [
        _t("pairs-clusters-meta", ["pairs"] + _I + ["--max-distance", "0.01", "--within", "{tmp}/within.txt", "--clusters", "-m"],
           stderr=True),
        _t("pairs-groups-summary", ["pairs"] + _I + ["--max-distance", "0.2", "--within", "{tmp}/within.txt", "--leave-out-groups",
                                                      "{tmp}/groups.tsv", "--summary-only", "--clusters"], stderr=True),
        _t("cluster-k", ["cluster"] + _I + ["-k", "3", "--seed", "5", "--within", "{tmp}/within.txt", "-m"], stderr=True),
        _t("cluster-init-ids", ["cluster"] + _I + ["--init-ids", "{tmp}/init.txt", "--within", "{tmp}/within.txt", "--summary-only", "-o",
                                                   "{tmp}/clusters.tsv"], stderr=True, outputs=["{tmp}/clusters.tsv"]),
        _t("cluster-whole-index", ["cluster"] + _I + ["-k", "4", "--summary-only", "--max-iterations", "5"]),
    ],
    "explain": [
        _t("explain-query-ids", ["explain"] + _I + _JF + ["--query-ids", "12,58", "-r", "3", "--top", "2"]),
        _t("explain-query-id-exact-meta", ["explain"] + _I + _JF + ["-q", "58", "-r", "3", "-e", "-m", "--summary-only"]),
        _t("explain-unhashed", ["explain"] + _I + _JF + ["-q", "58", "-r", "3", "--unhashed"]),
        _t("explain-unhashed-stream", ["explain"] + _I + _JF + ["-f", "raw", "-r", "3", "--unhashed"], _RAW),
        _t("explain-sample-within", ["explain"] + _I + _JF + ["--sample", "2", "--sample-seed", "4", "-r", "3", "--within",
                                                              "{tmp}/within.txt", "--summary-only"], stderr=True),
        _t("explain-stream", ["explain"] + _I + _JF + ["-f", "raw", "-r", "3"], _RAW),
        _t("explain-stream-exact", ["explain"] + _I + _JF + ["-f", "raw", "-r", "3", "-e"], _RAW),
        _t("explain-intropolis", ["explain"] + _I + _JF + ["--intropolis", _Q, "-r", "3", "--top", "2"]),
        _t("explain-intropolis-exact", ["explain"] + _I + _JF + ["--intropolis", _Q, "-r", "3", "-e", "--summary-only"]),
        _t("explain-against", ["explain"] + _I + _JF + ["--query-ids", "12,33", "--against", "33,58,24", "-m"]),
        _t("explain-against-stream", ["explain"] + _I + _JF + ["-f", "raw", "--against", "33,58"], _RAW),
        _t("explain-against-intropolis", ["explain"] + _I + _JF + ["--intropolis", _Q, "--against", "58,12", "--summary-only"]),
    ],
}


def _write_gz(path, text):
    with gzip.open(path, "wt") as fh:
        fh.write(text)


def _cli(argv, stdin_text=None):
    """(return code, stdout, stderr) of one command line; print() of the library's Python side included."""
    from morna_amd import cli
    out, err = io.StringIO(), io.StringIO()
    with contextlib.redirect_stdout(out), contextlib.redirect_stderr(err):
        rc = cli.main(argv, stdin=io.StringIO(stdin_text or ""), stdout=out)
    return rc, out.getvalue(), err.getvalue()


def build_transcript_index(tmp):
    """The index of tiny_intropolis.tsv (128 features, 4 trees, junction store, metadata) and the small files the command lines
    name, all in the directory tmp."""
    with open(os.path.join(HERE, "tiny_intropolis.tsv")) as fh:
        lines = fh.readlines()
    _write_gz(os.path.join(tmp, "tiny.tsv.gz"), "".join(lines))
    ids = sorted(set(int(i) for line in lines for i in line.split("\t")[6].split(",")))
    with open(os.path.join(tmp, "meta.tsv"), "w") as fh:
        fh.write("".join("%d\ttissue%d\trun%d\n" % (i, i % 5, i) for i in ids))
    heads = ["\t".join(line.split("\t")[:6]) for line in lines]
    _write_gz(os.path.join(tmp, "queries.gz"), heads[0] + "\t70000,70001\t3,1\n" + heads[1] + "\t70000\t5\n" + heads[2] + "\t70001\t2\n"
              + "chrUn\t1\t2\t+\tGT\tAG\t70001\t8\n")
    _write_gz(os.path.join(tmp, "truth.gz"), heads[0] + "\t70000,70001\t9,4\n" + heads[1] + "\t70000,70001\t12,1\n" + heads[2]
              + "\t70001\t6\n" + "chrUn\t1\t2\t+\tGT\tAG\t70000,70001\t3,8\n")
    files = {"within.txt": "".join("%d\n" % i for i in _WITHIN), "without.txt": "1\n3\n5\n",
             "groups.tsv": "donorA\t12,20,51\ndonorB\t33,58,43\n", "pools.tsv": "first\t12,20,51,58\nsecond\t24,56\n",
             "labels.tsv": "".join("tissue%d\t%s\n" % (t, ",".join(str(i) for i in _WITHIN[t::3])) for t in range(3)),
             "init.txt": "12\n24\n58\n", "pass1.sam": _SAM}
    for name, text in files.items():
        with open(os.path.join(tmp, name), "w") as fh:
            fh.write(text)
    rc = _cli(["index", "--intropolis", os.path.join(tmp, "tiny.tsv.gz"), "-x", os.path.join(tmp, "idx"), "--features", "128",
               "--n-trees", "4", "-t", "100", "-m", os.path.join(tmp, "meta.tsv"), "--junction-store"])[0]
    assert rc == 0


def run_transcript(case, tmp):
    """One command line on the index build_transcript_index left in tmp: its return code (or exception), stdout, stderr and
    written files where the case names them, with tmp written as {tmp}."""
    try:
        rc, out, err = _cli([a.replace("{tmp}", tmp) for a in case["argv"]], case["stdin"])
        got = {"rc": rc, "stdout": out}
        if case["stderr"]:
            got["stderr"] = err
    except Exception as e:                                     # noqa: BLE001
        got = {"raises": type(e).__name__, "text": str(e)}
    got["files"] = {}
    for path in case["outputs"]:
        with open(path.replace("{tmp}", tmp)) as fh:
            got["files"][path] = fh.read()
    return json.loads(json.dumps(got).replace(tmp, "{tmp}"))


def _json_lines(value, pad, width=1000):
    """value as JSON lines: on one line where that takes at most `width` characters, a line per member otherwise."""
    text = json.dumps(value, sort_keys=True)
    if len(text) <= width or not isinstance(value, (list, dict)):
        return [pad + text]
    if isinstance(value, list):
        members, brackets = [_json_lines(v, pad + " ", width) for v in value], "[]"
    else:
        members, brackets = [], "{}"
        for key in sorted(value):
            lines = _json_lines(value[key], pad + " ", width)
            members.append([pad + " " + json.dumps(key) + ": " + lines[0].lstrip()] + lines[1:])
    for lines in members[:-1]:
        lines[-1] += ","
    return [pad + brackets[0]] + [line for lines in members for line in lines] + [pad + brackets[1]]


def _dump(path, data):
    with open(path, "w") as fh:
        fh.write("\n".join(_json_lines(data, "")) + "\n")


def main():
    import tempfile
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--transcripts", metavar="<file>", default=None, help="write the transcripts here instead (needs the GPU)")
    opts = ap.parse_args()
    if opts.transcripts is not None:
        with tempfile.TemporaryDirectory() as tmp:
            build_transcript_index(tmp)
            _dump(opts.transcripts, dict((group, [dict(case, result=run_transcript(case, tmp)) for case in cases])
                                         for group, cases in TRANSCRIPT_GROUPS.items()))
        return
    _dump(PARSER_JSON, parser_structure())
    refusals = []
    for case in REFUSAL_CASES:
        with tempfile.TemporaryDirectory() as tmp:
            refusals.append(dict(case, outcome=run_refusal(case, tmp)))
    _dump(REFUSALS_JSON, refusals)


if __name__ == "__main__":
    main()
