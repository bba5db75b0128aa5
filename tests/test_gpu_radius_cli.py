"""search -e --max-distance and `morna pairs` on the command line, on the synthetic 600-sample cohort of the
other command-line tests.  The blocks of a stream, --intropolis and --within query are the `search -e -r 600` blocks cut at
the distance; -q and --query-ids, which `-e` does not reach today, are compared with the exact search by item printed the
same way; the pairs with the lists `search` printed.  Whole text.  -m gpu"""
import io
import re

import numpy as np
import pytest

from test_gpu_junctions import blocks, result_ids, run_cli

pytestmark = pytest.mark.gpu

N_INDEX, N_QUERY, J, THRESHOLD, TREES, DIM = 600, 12, 3000, 30, 5, 128


@pytest.fixture(scope="module")
def cohort(tmp_path_factory):
    from morna_amd.search import MornaSearch
    from morna_amd.synth import index_and_query_files
    d = tmp_path_factory.mktemp("radius_cohort")
    ipath, qpath = str(d / "index.tsv.gz"), str(d / "queries.tsv")
    made = index_and_query_files(ipath, qpath, N_INDEX, N_QUERY, J=J)
    base = str(d / "idx")
    with open(str(d / "meta.tsv"), "w") as fh:                 # every sample but the first has keywords
        fh.write("".join("%d\ttissue%d adult\n" % (s, s % 3) for s in sorted(int(x) for x in made["index_ids"])[1:]))
    assert run_cli(["index", "--intropolis", ipath, "-x", base, "--features", str(DIM), "--n-trees", str(TREES), "-t", str(THRESHOLD),
                    "-m", str(d / "meta.tsv")])[0] == 0
    searcher = MornaSearch(base)
    ids = sorted(searcher.internal_id_map)
    assert len(ids) == N_INDEX
    inv = {v: k for k, v in searcher.internal_id_map.items()}
    # the exact lists of every indexed sample, k = n_items (the GPU yardstick), and a distance that pairs about 150 of them
    items = np.arange(N_INDEX, dtype=np.int32)
    full = searcher.annoy_index.exact_search_by_item_batch(items, N_INDEX)
    assert (full[2] == N_INDEX).all()
    off = np.sort(full[1][full[0] != items[:, None]])
    some = ids[::3]
    with open(str(d / "some.txt"), "w") as fh:
        fh.write("".join("%d\n" % s for s in some))
    return dict(dir=d, base=base, queries_file=qpath, ids=ids, id_map=searcher.internal_id_map, inv=inv, full=full,
                pair_distance=float(off[299]), some=some, some_file=str(d / "some.txt"), searcher=searcher)


_LINE = re.compile(r"^\d+\.\t(-?\d+)\t(\S+)")


def cut_block(body, distance, cap=None):
    """The block with its result lines kept while their printed distance is <= distance (at most cap of them)."""
    out, n = [], 0
    for line in body.splitlines(True):
        m = _LINE.match(line)
        if not m:
            out.append(line)
        elif float(m.group(2)) <= distance and (cap is None or n < cap):
            n += 1
            out.append(line)
    return "".join(out)


def kth_distance(full_text, k):
    """The median over the blocks of the k-th printed distance: a radius that cuts every block somewhere else."""
    ds = [float(_LINE.match(body.splitlines()[k - 1]).group(2)) for _, body in blocks(full_text)]
    return sorted(ds)[len(ds) // 2]


@pytest.mark.parametrize("extra", [[], ["--within"]], ids=["all", "within"])
def test_intropolis_blocks_are_the_full_blocks_cut_at_the_distance(cohort, extra):
    extra = extra + [cohort["some_file"]] if extra else []
    common = ["search", "-x", cohort["base"], "-e", "-d", "--intropolis", cohort["queries_file"]] + extra
    rc, full, _ = run_cli(common + ["-r", str(N_INDEX)])
    assert rc == 0 and len(blocks(full)) == N_QUERY
    for distance in (kth_distance(full, 10), 0.0, 2.5):
        rc, got, _ = run_cli(common + ["--max-distance", repr(distance)])
        assert rc == 0
        want = "".join("# query %d\n%s" % (q, cut_block(body, distance)) for q, body in blocks(full))
        assert got == want, distance
    distance = kth_distance(full, 10)
    lens = [len(result_ids(body)) for _, body in blocks(run_cli(common + ["--max-distance", repr(distance)])[1])]
    assert min(lens) < 10 <= max(lens)                             # the distance cuts the blocks, not a result count
    # -r, when given, is a cap
    rc, capped, _ = run_cli(common + ["--max-distance", repr(distance), "-r", "4"])
    assert rc == 0 and capped == "".join("# query %d\n%s" % (q, cut_block(body, distance, 4)) for q, body in blocks(full))


def test_a_stream_query(cohort):
    """One query from a stream (-f raw): the -e block cut at the distance."""
    with open(cohort["queries_file"]) as fh:
        lines = [l.split("\t") for l in fh.read().splitlines()]
    first = lines[0][-2].split(",")[0]
    raw = "".join("%s\t%s\t%s\t%s\n" % (t[0], t[1], t[2], c) for t in lines
                  for smp, c in zip(t[-2].split(","), t[-1].split(",")) if smp == first)
    common = ["search", "-x", cohort["base"], "-e", "-d", "-f", "raw"]
    rc, full, _ = run_cli(common + ["-r", str(N_INDEX)], raw)
    assert rc == 0 and len(result_ids(full)) == N_INDEX
    distance = float(_LINE.match(full.splitlines()[14]).group(2))
    rc, got, _ = run_cli(common + ["--max-distance", repr(distance)], raw)
    assert rc == 0 and got == cut_block(full, distance) and len(result_ids(got)) >= 15


def _member_text(cohort, query_ids, distance, numbered, cap=None):
    """What -q / --query-ids print for the exact by-item lists (k = n_items) cut at the distance."""
    from morna_amd.search import results_output
    ids, d, _ = cohort["full"]
    out = io.StringIO()
    for s in query_ids:
        q = cohort["id_map"][s]
        if numbered:
            out.write("# query %d\n" % s)
        out.write("querying by sample id %d\nthis is internal id %d\n" % (s, q))
        keep = d[q] <= distance
        results_output(([int(x) for x in ids[q][keep]][:cap], [float(x) for x in d[q][keep]][:cap]), out)
    return out.getvalue()


def test_by_sample_blocks_are_the_exact_by_item_lists_cut_at_the_distance(cohort):
    ids = cohort["ids"]
    queries = [ids[5], ids[311], ids[77]]
    distance = float(np.median(cohort["full"][1][[cohort["id_map"][s] for s in queries], 12]))
    rc, got, _ = run_cli(["search", "-x", cohort["base"], "-e", "-d", "--max-distance", repr(distance), "--query-ids",
                          ",".join(map(str, queries))])
    assert rc == 0 and got == _member_text(cohort, queries, distance, True)
    rc, got, _ = run_cli(["search", "-x", cohort["base"], "-e", "-d", "--max-distance", repr(distance), "-q", str(queries[1])])
    assert rc == 0 and got == _member_text(cohort, [queries[1]], distance, False)
    rc, got, _ = run_cli(["search", "-x", cohort["base"], "-e", "-d", "--max-distance", repr(distance), "-q", str(queries[1]), "-r", "2"])
    assert rc == 0 and got == _member_text(cohort, [queries[1]], distance, False, cap=2)
    with pytest.raises(ValueError, match="Querying sample id 999999"):
        run_cli(["search", "-x", cohort["base"], "-e", "--max-distance", "0.5", "-q", "999999"])


def test_search_without_the_flag_is_unchanged(cohort):
    """-e without --max-distance prints what the exact search of the library returns, -r deep, as before."""
    from morna_amd.search import results_output
    searcher = cohort["searcher"]
    batch = searcher.queries_from_intropolis(cohort["queries_file"])
    out = io.StringIO()
    for sample_id, res in zip(batch.ext_ids, searcher.exact_search_nn_batch(batch, 20)):
        out.write("# query %d\n" % sample_id)
        results_output(res, out)
    rc, got, _ = run_cli(["search", "-x", cohort["base"], "-e", "-d", "--intropolis", cohort["queries_file"]])
    assert rc == 0 and got == out.getvalue()
    rc, given, _ = run_cli(["search", "-x", cohort["base"], "-e", "-d", "--intropolis", cohort["queries_file"], "-r", "20"])
    assert rc == 0 and given == got


def _printed_pairs(cohort, distance):
    """The pairs the lists `search -e --max-distance` prints for every indexed sample hold: (idA, idB) -> distance text."""
    rc, text, _ = run_cli(["search", "-x", cohort["base"], "-e", "-d", "--max-distance", repr(distance), "--query-ids",
                           ",".join(map(str, cohort["ids"]))])
    assert rc == 0
    pairs = {}
    for s, body in blocks(text):
        for line in body.splitlines():
            m = _LINE.match(line)
            if m and cohort["inv"][int(m.group(1))] != s:
                other = cohort["inv"][int(m.group(1))]
                key = (min(s, other), max(s, other))
                assert pairs.setdefault(key, m.group(2)) == m.group(2)       # printed from both ends, the same text
    return pairs


def test_pairs_lines_and_summary_against_the_printed_lists(cohort):
    from morna_amd.search import pair_clusters
    distance = cohort["pair_distance"]
    want = _printed_pairs(cohort, distance)
    assert 100 <= len(want) <= 400
    rc, got, _ = run_cli(["pairs", "-x", cohort["base"], "--max-distance", repr(distance), "--clusters"])
    assert rc == 0
    lines = got.splitlines()
    pair_lines = [l for l in lines if not l.startswith("#")]
    assert len(pair_lines) == len(want)
    parsed = [(int(a), int(b), t) for a, b, t in (l.split("\t") for l in pair_lines)]
    assert all(a < b for a, b, _ in parsed) and {(a, b): t for a, b, t in parsed} == want
    assert [(float(t), a, b) for a, b, t in parsed] == sorted((float(t), a, b) for a, b, t in parsed)
    clusters = pair_clusters(parsed)
    assert lines[len(pair_lines)] == "# samples %d\tpairs %d\tsamples in any pair %d\tlargest cluster %d" % (
        N_INDEX, len(want), len(set(i for a, b, _ in parsed for i in (a, b))), len(clusters[0]))
    assert lines[len(pair_lines) + 1:] == ["# cluster %d\t%s" % (len(c), ",".join(map(str, c))) for c in clusters]
    rc, short, _ = run_cli(["pairs", "-x", cohort["base"], "--max-distance", repr(distance), "--summary-only"])
    assert rc == 0 and short == lines[len(pair_lines)] + "\n"
    # -m: both samples' keywords, "-" for a sample the metafile does not name
    rc, meta, _ = run_cli(["pairs", "-x", cohort["base"], "--max-distance", repr(distance), "-m"])
    first_id = cohort["ids"][0]
    word = lambda s: "-" if s == first_id else "tissue%d adult" % (s % 3)
    assert rc == 0 and meta.splitlines()[:len(pair_lines)] == ["%s\t%s\t%s" % (l, word(a), word(b)) for l, (a, b, _) in zip(pair_lines, parsed)]
    # --within: only pairs of listed samples; --leave-out-groups: never two samples of one group, the rest unchanged
    some = set(cohort["some"])
    rc, got, err = run_cli(["pairs", "-x", cohort["base"], "--max-distance", repr(distance), "--within", cohort["some_file"]])
    inside = {k: t for k, t in want.items() if k[0] in some and k[1] in some}
    assert rc == 0 and "restriction: %d of %d samples allowed" % (len(some), N_INDEX) in err
    assert {(int(a), int(b)): t for a, b, t in (l.split("\t") for l in got.splitlines() if not l.startswith("#"))} == inside
    assert got.splitlines()[-1].startswith("# samples %d\tpairs %d\t" % (len(some), len(inside)))
    first = sorted(want)[:40]
    members = sorted(set(i for k in first for i in k))
    gfile = str(cohort["dir"] / "donors.tsv")
    with open(gfile, "w") as fh:
        fh.write("donorA\t%s\n" % ",".join(map(str, members)))
    rc, got, _ = run_cli(["pairs", "-x", cohort["base"], "--max-distance", repr(distance), "--leave-out-groups", gfile])
    silent = {k: t for k, t in want.items() if not (k[0] in members and k[1] in members)}
    assert rc == 0 and len(silent) <= len(want) - 40
    assert {(int(a), int(b)): t for a, b, t in (l.split("\t") for l in got.splitlines() if not l.startswith("#"))} == silent
