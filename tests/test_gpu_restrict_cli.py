"""--within / --without / --leave-out-groups on the command line, on a synthetic cohort with a junction
store: `search` blocks against the full-depth unrestricted lists filtered on the host, `recovery` tables against the
set-and-dict restatement fed the lists the restricted search printed, `junctions` splice files against the restatement.
Whole text.  -m gpu"""
import gzip
import os
import re

import pytest

from test_gpu_junctions import blocks, read, result_ids, run_cli
from test_gpu_recovery import summary_text, table_text
from test_junctions_cpu import ref_junctions, sample_lists
from test_recovery_cpu import ref_recovery, rows_of_tables

pytestmark = pytest.mark.gpu

N_INDEX, N_QUERY, J, THRESHOLD, TREES, DIM = 600, 12, 3000, 30, 5, 128


@pytest.fixture(scope="module")
def cohort(tmp_path_factory):
    from morna_amd.search import MornaSearch
    from morna_amd.synth import index_and_query_files
    d = tmp_path_factory.mktemp("restrict_cohort")
    ipath, qpath = str(d / "index.tsv.gz"), str(d / "queries.tsv")
    index_and_query_files(ipath, qpath, N_INDEX, N_QUERY, J=J)
    base = str(d / "idx")
    with gzip.open(ipath, "rt") as fh:
        lines = fh.readlines()
    tables = sample_lists(lines)
    rows = rows_of_tables(tables)
    assert run_cli(["index", "--intropolis", ipath, "-x", base, "--features", str(DIM), "--n-trees", str(TREES), "-t", str(THRESHOLD),
                    "--junction-store"])[0] == 0
    searcher = MornaSearch(base)
    id_map = searcher.internal_id_map
    ids = sorted(id_map)
    assert len(ids) == N_INDEX

    def write(name, text):
        with open(str(d / name), "w") as fh:
            fh.write(text)
        return str(d / name)
    some = ids[::3]                                            # a third of the index
    queries = [ids[5], ids[311], ids[77]]
    # the first query in a group of 40 with the three samples the search puts nearest to it (leaving them out shows in every
    # table), the second in a group of 2, the third not named
    inv = {v: k for k, v in id_map.items()}
    _, nearest = searcher.search_member_n_batch([queries[0]], 4, 100, include_distances=False)
    near = [inv[i] for i in nearest[0][0] if inv[i] != queries[0]][:3]
    donor = [queries[0]] + near + [s for s in ids[100:150] if s not in near and s not in queries][:36]
    assert len(donor) == 40 and len(set(donor)) == 40
    groups = [("donorA", donor), ("donorB", [queries[1], ids[400]]), ("lonely", [ids[500]])]
    return dict(dir=d, base=base, index=ipath, queries_file=qpath, lines=lines, tables=tables, rows=rows, ids=ids, id_map=id_map,
                inv={v: k for k, v in id_map.items()}, some=some, queries=queries, groups=groups,
                some_file=write("some.txt", "".join("%d\n" % s for s in some)),
                groups_file=write("groups.tsv", "".join("%s\t%s\n" % (label, ",".join(map(str, g))) for label, g in groups)),
                singles_file=write("singles.tsv", "".join("q%d\t%d\n" % (s, s) for s in queries)))


_LINE = re.compile(r"^\d+\.(\t.*)$")


def filtered(body, keep, k):
    """The result lines of a block whose internal id `keep` accepts, the first k, numbered anew; other lines as they are."""
    out, n = [], 0
    for line in body.splitlines(True):
        m = _LINE.match(line.rstrip("\n"))
        if not m:
            out.append(line)
            continue
        if keep(int(m.group(1).split("\t")[1])) and n < k:
            n += 1
            out.append("%d.%s\n" % (n, m.group(1)))
    return "".join(out)


@pytest.mark.parametrize("mode", [["-e"], ["--search-k", "300"], ["--unhashed"]], ids=["exact", "approximate", "unhashed"])
@pytest.mark.parametrize("flag", ["--within", "--without"])
def test_search_equals_the_filtered_full_depth_search(cohort, mode, flag):
    query = (["--query-ids", ",".join(map(str, cohort["queries"]))] if mode == ["--unhashed"]
             else ["--intropolis", cohort["queries_file"]])
    common = ["search", "-x", cohort["base"], "-d"] + query + mode
    rc, got, err = run_cli(common + [flag, cohort["some_file"], "-r", "5"])
    assert rc == 0
    n_allowed = len(cohort["some"]) if flag == "--within" else N_INDEX - len(cohort["some"])
    assert "restriction: %d of %d samples allowed, 0 leave-out groups\n" % (n_allowed, N_INDEX) in err
    rc, full, _ = run_cli(common + ["-r", str(N_INDEX)])
    assert rc == 0
    listed = set(cohort["id_map"][s] for s in cohort["some"])
    keep = (lambda i: i in listed) if flag == "--within" else (lambda i: i not in listed)
    got_blocks, full_blocks = blocks(got), blocks(full)
    assert [q for q, _ in got_blocks] == [q for q, _ in full_blocks] and len(got_blocks) >= 3
    for (q, body), (_, whole) in zip(got_blocks, full_blocks):
        assert body == filtered(whole, keep, 5), (mode, flag, q)
        assert len(result_ids(body)) == 5 and all(keep(i) for i in result_ids(body))
    assert got != "".join("# query %d\n%s" % (q, filtered(whole, lambda i: True, 5)) for q, whole in full_blocks)


def test_search_k_default_grows_under_an_allow_list(cohort):
    """Without --search-k an allow-list of a third searches with n_trees * r * 3; an explicit --search-k is taken as given."""
    common = ["search", "-x", cohort["base"], "-d", "--query-ids", ",".join(map(str, cohort["queries"]))]
    rc, got, _ = run_cli(common + ["--within", cohort["some_file"], "-r", "5"])
    rc2, given, _ = run_cli(common + ["--within", cohort["some_file"], "-r", "5", "--search-k", str(TREES * 5 * 3)])
    assert rc == 0 and rc2 == 0 and got == given
    rc, hundred, _ = run_cli(common + ["--within", cohort["some_file"], "-r", "5", "--search-k", "100"])
    rc2, full, _ = run_cli(common + ["-r", str(N_INDEX), "--search-k", "100"])
    listed = set(cohort["id_map"][s] for s in cohort["some"])
    assert rc == 0 and rc2 == 0
    for (q, body), (_, whole) in zip(blocks(hundred), blocks(full)):
        assert body == filtered(whole, lambda i: i in listed, 5), q


def own_group(cohort, q):
    for _, members in cohort["groups"]:
        if q in members:
            return set(cohort["id_map"][s] for s in members)
    return {cohort["id_map"][q]}


@pytest.mark.parametrize("single", [False, True], ids=["query_ids", "q"])
def test_search_leaves_the_query_s_group_out(cohort, single):
    queries = cohort["queries"][:1] if single else cohort["queries"]
    query = ["-q", str(queries[0])] if single else ["--query-ids", ",".join(map(str, queries))]
    common = ["search", "-x", cohort["base"], "-d", "--search-k", "400"] + query
    rc, got, err = run_cli(common + ["--leave-out-groups", cohort["groups_file"], "-r", "10"])
    assert rc == 0
    n_groups = 3 + (0 if single else 1)                         # the third query is a group of its own
    assert "restriction: %d of %d samples allowed, %d leave-out groups\n" % (N_INDEX, N_INDEX, n_groups) in err
    rc, full, _ = run_cli(common + ["-r", str(N_INDEX)])
    assert rc == 0
    got_blocks = [(queries[0], got)] if single else blocks(got)
    full_blocks = [(queries[0], full)] if single else blocks(full)
    assert [q for q, _ in got_blocks] == queries
    changed = 0
    for (q, body), (_, whole) in zip(got_blocks, full_blocks):
        out = own_group(cohort, q)
        assert not set(result_ids(body)) & out and len(result_ids(body)) == 10
        assert body == filtered(whole, lambda i: i not in out, 10), q
        assert cohort["id_map"][q] in result_ids(filtered(whole, lambda i: True, 10))      # without the flag the query finds itself
        changed += len(set(result_ids(filtered(whole, lambda i: True, 10))) & out)
    assert changed >= len(queries)


def recovery_flags(cohort):
    return ["-x", cohort["base"], "--query-ids", ",".join(map(str, cohort["queries"]))]


def test_recovery_leave_out_groups_equals_restatement(cohort):
    from morna_amd.junctions import parse_recovery_grid
    frequencies, coverages = parse_recovery_grid()
    groups = ["--leave-out-groups", cohort["groups_file"]]
    rc, out, _ = run_cli(["recovery", "-r", "5"] + recovery_flags(cohort) + groups)
    assert rc == 0
    rc, searched, _ = run_cli(["search", "-r", "5"] + recovery_flags(cohort) + groups)      # exactly -r: nothing to drop
    assert rc == 0
    texts, tables = [], []
    for q, body in blocks(searched):
        results = [cohort["inv"][i] for i in result_ids(body)]
        assert len(results) == 5 and not set(result_ids(body)) & own_group(cohort, q)
        line, cov = cohort["rows"][q]
        truth = line[cov >= 1].tolist()
        text, rows = table_text(cohort["rows"], len(cohort["lines"]), q, results, truth, 0, frequencies, coverages)
        retrieved, tp, true = ref_recovery(cohort["lines"], results, truth, float(frequencies[1]), coverages[1], cohort["tables"])
        at = len(coverages) + 1
        assert (rows[at]["retrieved"], rows[at]["true_positive"], rows[at]["false_negative"]) == (retrieved, tp, true - tp)
        texts.append(text)
        tables.append(rows)
    assert len(texts) == 3 and out == "".join(texts) + summary_text(tables)
    rc, plain, _ = run_cli(["recovery", "-r", "5"] + recovery_flags(cohort))
    assert rc == 0 and plain != out                            # leaving the donors out changes the tables


@pytest.mark.parametrize("extra", [[], ["--results-sweep", "2,5"], ["--downsample", "0.5,0.1"], ["--downsample", "0.5", "-e"]],
                         ids=["plain", "sweep", "downsample", "downsample_exact"])
def test_recovery_with_singleton_groups_is_today_s_recovery(cohort, extra):
    """Every query a group of its own: the search leaves out what `recovery` drops today, so every byte is the same -- with a
    groups file that names the queries, and with one that names nobody (a query the file does not name is its own group)."""
    flags = ["recovery", "-r", "5"] + recovery_flags(cohort) + extra
    if "--downsample" in extra:
        flags += ["--junction-file", cohort["index"]]
    rc, today, _ = run_cli(flags)
    assert rc == 0
    rc, single, err = run_cli(flags + ["--leave-out-groups", cohort["singles_file"]])
    assert rc == 0 and single == today
    assert "restriction: %d of %d samples allowed, 3 leave-out groups" % (N_INDEX, N_INDEX) in err
    empty = str(cohort["dir"] / "nobody.tsv")
    with open(empty, "w") as fh:
        fh.write("nobody\t\n")
    rc, implied, _ = run_cli(flags + ["--leave-out-groups", empty])
    assert rc == 0 and implied == today


@pytest.mark.parametrize("extra", [["--results-sweep", "2,5"], ["--downsample", "0.5,0.1"]], ids=["sweep", "downsample"])
def test_recovery_leave_out_groups_composes(cohort, extra):
    """--results-sweep: the prefixes of a restricted list are restricted lists, so every count's tables are those of a run
    of its own.  --downsample: the thinned queries leave their sample's group out -- the lists `search --downsample` prints under
    the same flags, tabulated by the restatement."""
    from morna_amd.junctions import parse_recovery_grid
    from test_gpu_recovery_sweep import headed_blocks
    frequencies, coverages = parse_recovery_grid()
    groups = ["--leave-out-groups", cohort["groups_file"]]
    if extra[0] == "--results-sweep":
        rc, out, _ = run_cli(["recovery", "-r", "5"] + recovery_flags(cohort) + groups + extra)
        assert rc == 0
        got = headed_blocks(out)
        for i, p in enumerate((2, 5)):
            rc, alone, _ = run_cli(["recovery", "-r", str(p)] + recovery_flags(cohort) + groups)
            separate = headed_blocks(alone)
            assert rc == 0 and len(separate) == 4
            for j in range(3):
                assert got[2 * j + i] == separate[j], (p, j)
            assert got[6 + i][1] == separate[3][1], p
        return
    flags = recovery_flags(cohort) + groups + extra + ["--junction-file", cohort["index"]]
    rc, out, _ = run_cli(["recovery", "-r", "5"] + flags)
    assert rc == 0
    rc, searched, _ = run_cli(["search", "-r", "5"] + flags)
    assert rc == 0
    parts = re.split(r"^# query (-?\d+)\tkeep (\S+)\n", searched, flags=re.M)
    found = [((int(parts[i]), parts[i + 1]), parts[i + 2]) for i in range(1, len(parts), 3)]
    assert [job for job, _ in found] == [(q, rate) for q in cohort["queries"] for rate in ("0.5", "0.1")]
    got = [b for b in headed_blocks(out) if b[0].startswith("# query")]
    assert len(got) == len(found)
    for ((q, rate), body), (head, table) in zip(found, got):
        results = [cohort["inv"][i] for i in result_ids(body)]
        assert len(results) == 5 and not set(result_ids(body)) & own_group(cohort, q)
        line, cov = cohort["rows"][q]
        truth = line[cov >= 1].tolist()
        text, _ = table_text(cohort["rows"], len(cohort["lines"]), q, results, truth, 0, frequencies, coverages)
        assert head == "# query %d\tkeep %s\tresults 5\ttrue %d\n" % (q, rate, len(truth))
        assert table == text.split("\n", 1)[1], (q, rate)


def test_junctions_within_equals_restatement(cohort, tmp_path):
    sf = str(tmp_path / "splices")
    listed = set(cohort["id_map"][s] for s in cohort["some"])
    rc, out, _ = run_cli(["junctions", "-x", cohort["base"], "--junction-file", cohort["index"], "-sf", sf, "--junction-filter", ".2,40",
                          "--query-ids", ",".join(map(str, cohort["queries"])), "--within", cohort["some_file"], "-r", "8"])
    assert rc == 0
    found = blocks(out)
    assert [q for q, _ in found] == cohort["queries"]
    for q, body in found:
        results = result_ids(body)
        assert len(results) == 8 and set(results) <= listed
        want = ref_junctions(cohort["lines"], [cohort["inv"][i] for i in results], 0.2, 40, cohort["tables"])
        assert read(sf + "." + str(q)) == want["text"], q
        assert "Number of retained junctions: %d\n" % want["count"] in out


def test_unknown_ids_and_sharded_sets_are_refused(cohort, tmp_path):
    bad = str(tmp_path / "bad.txt")
    with open(bad, "w") as fh:
        fh.write("%d\n424242\n" % cohort["ids"][0])
    with pytest.raises(ValueError, match="424242"):
        run_cli(["search", "-x", cohort["base"], "-q", str(cohort["queries"][0]), "--within", bad])
    two = str(tmp_path / "two.tsv")
    with open(two, "w") as fh:
        fh.write("a\t%d,%d\nb\t%d\n" % (cohort["ids"][0], cohort["ids"][1], cohort["ids"][1]))
    with pytest.raises(ValueError, match=str(cohort["ids"][1])):
        run_cli(["search", "-x", cohort["base"], "-q", str(cohort["queries"][0]), "--leave-out-groups", two])
    # without the flags: the bytes of before (the same command twice, and the restriction left no trace in the searcher)
    plain = ["search", "-x", cohort["base"], "-d", "-q", str(cohort["queries"][0])]
    assert run_cli(plain) == run_cli(plain)
    from morna_amd.search import SHARDS_REFUSAL
    base = str(tmp_path / "sharded")
    assert run_cli(["index", "--intropolis", cohort["index"], "-x", base, "--features", str(DIM), "--n-trees", "2", "-t", str(THRESHOLD),
                    "--shards", "2"])[0] == 0
    assert os.path.exists(base + ".shards.mor")
    with pytest.raises(ValueError) as e:
        run_cli(["search", "-x", base, "-q", str(cohort["queries"][0]), "--within", cohort["some_file"]])
    assert str(e.value) == SHARDS_REFUSAL
