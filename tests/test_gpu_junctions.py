"""`morna index --junction-store` and `morna junctions` on the GPU: the store's content and determinism, and whole splice
files against the restatement of morna.py:1539-1629 (test_junctions_cpu.ref_junctions), fed the result lists the search
itself returned -- so the junction logic is pinned, not neighbour order or ties.  Every comparison is of whole files or
whole arrays, byte for byte.  -m gpu"""
import contextlib
import gzip
import io
import os
import re

import pytest

from test_junctions_cpu import ref_junctions, ref_retain, sample_lists, tiny_lines

pytestmark = pytest.mark.gpu

FILTERS = [".05,5", ".5,3", "1.0,1000", "0,1000"]
N_INDEX, N_QUERY, J, THRESHOLD, TREES, DIM = 3000, 300, 12000, 30, 10, 256


def _write_gz(path, lines):
    with gzip.open(path, "wt") as fh:
        fh.write("".join(lines))


def run_cli(argv, stdin_text=None):
    """(return code, stdout, stderr) of one command line; print() of the library's Python side included."""
    from morna_amd import cli
    out, err = io.StringIO(), io.StringIO()
    with contextlib.redirect_stdout(out), contextlib.redirect_stderr(err):
        rc = cli.main(argv, stdin=io.StringIO(stdin_text or ""), stdout=out)
    return rc, out.getvalue(), err.getvalue()


_RESULT = re.compile(r"^\d+\.\t(-?\d+)(\t|$)", re.M)


def result_ids(text):
    """Internal ids of the result lines results_output wrote."""
    return [int(m.group(1)) for m in _RESULT.finditer(text)]


def blocks(text):
    parts = re.split(r"^# query (-?\d+)\n", text, flags=re.M)
    return [(int(parts[i]), parts[i + 1]) for i in range(1, len(parts), 2)]


def read(path):
    with open(path) as fh:
        return fh.read()


def parts_of(filt):
    f, c = filt.split(",")
    return float(f), int(c)


def check_single(base, lines, tables, src, tmp, query_flags, filt, stdin_text=None, search_flags=None):
    """One `junctions` run with one query: stdout is `search`'s and then the count, stderr the reference's line, the splice
    file the restatement's for the results printed.  Returns the restatement's answer."""
    from morna_amd.search import MornaSearch
    sf = str(tmp / ("splices_%d" % len(os.listdir(str(tmp)))))
    rc, out, err = run_cli(["junctions", "-x", base, "--junction-file", src, "-sf", sf, "--junction-filter", filt] + query_flags,
                           stdin_text)
    assert rc == 0
    _, want_out, _ = run_cli(["search", "-x", base] + (search_flags if search_flags is not None else query_flags), stdin_text)
    inv = {v: k for k, v in MornaSearch(base).internal_id_map.items()}
    results = [inv[i] for i in result_ids(want_out)]
    ref = ref_junctions(lines, results, *parts_of(filt), tables=tables)
    assert out == want_out + "Number of retained junctions: %d\n" % ref["count"]
    assert err.endswith("%d junctions to begin with\n" % ref["count"])
    assert read(sf) == ref["text"]
    return ref, results


# ---- the embedded fixture ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def generic(tmp_path_factory, embedded):
    d = tmp_path_factory.mktemp("generic")
    src, base = str(d / "junctions.gz"), str(d / "idx")
    _write_gz(src, embedded["generic"])
    rc, _, _ = run_cli(["index", "--intropolis", src, "-x", base, "--features", "128", "--n-trees", "5", "-s", "10", "-t", "4",
                        "--junction-store"])
    assert rc == 0
    return dict(dir=d, src=src, base=base, lines=embedded["generic"], tables=sample_lists(embedded["generic"]))


def test_generic_index_holds_3_lines_and_the_store_all_20(generic):
    from morna_amd.junctions import JunctionStore
    from morna_amd.search import MornaSearch
    s = MornaSearch(generic["base"])
    assert len(s.sample_frequencies) == 3 and s.index_size == 10
    store = JunctionStore.load(generic["base"] + ".junc.mor")
    juncs, covrs = generic["tables"]
    assert (store.n_samples, store.n_lines, store.nnz) == (10, 20, sum(len(v) for v in juncs.values()))
    assert store.sample_ids().tolist() == list(juncs)                       # first-seen order over ALL lines
    for sample in juncs:
        line, cov = store.sample(sample)
        assert line.tolist() == juncs[sample] and cov.tolist() == [int(c) for c in covrs[sample]]


@pytest.mark.parametrize("filt", FILTERS)
def test_generic_q_runs_equal_restatement(generic, tmp_path, filt):
    nonempty = 0
    for sample in range(1, 11):
        ref, _ = check_single(generic["base"], generic["lines"], generic["tables"], generic["src"], tmp_path,
                              ["-q", str(sample), "-r", "5"], filt)
        nonempty += ref["count"] > 0
    assert nonempty == 10                                                   # line 16 is in every sample


def test_generic_min_count_3_of_7_and_api(generic, tmp_path):
    """f = 0.3 with 7 results: ceil(2.1) = 3; and MornaSearch.retain_junctions' objects."""
    from morna_amd.search import MornaSearch
    ref, results = check_single(generic["base"], generic["lines"], generic["tables"], generic["src"], tmp_path,
                                ["-q", "8", "-r", "7", "-d"], ".3,1000")
    assert len(results) == 7
    s = MornaSearch(generic["base"])
    internal = [s.internal_id_map[x] for x in results]
    kept, none = s.retain_junctions([internal, []], 0.3, 1000)
    assert kept.lines.tolist() == ref["lines"] and kept.found_in == ref["found_in"] and kept.coverages == ref["covs"]
    assert len(none) == 0 and none.found_in == [] and none.coverages == []
    for f, c in ((0, 10**12), (1.0, 10**12), (0.05, 5), (-1.0, 3), (2.0, 3), (0.5, -7)):
        kept = s.retain_junctions([internal[:m] for m in (7, 1, 4)], f, c)
        for m, got in zip((7, 1, 4), kept):
            want = ref_junctions(generic["lines"], results[:m], f, c, tables=generic["tables"])
            assert (got.lines.tolist(), got.found_in, got.coverages) == (want["lines"], want["found_in"], want["covs"]), (f, c, m)
    with pytest.raises(IndexError, match="424242"):
        s.junction_store().retain([[1, 424242]], .05, 5)


def test_generic_sam_query_is_read_from_pass1_sam(generic, tmp_path):
    """No query flag: the SAM file named by -p1 is the query, in place of stdin (morna.py:1351-1353)."""
    from morna_amd.index import tokenize_line
    sam = []
    for ln in generic["lines"]:
        key, samples, cov = tokenize_line(ln)
        if 8 in samples:
            chrom, start, end = key.split(" ")
            for _ in range(cov[samples.index(8)]):
                sam.append("r\t0\t%s\t%d\t255\t10M%dN10M\t*\t0\t0\t*\t*\n" % (chrom, int(start) - 10, int(end) - int(start) + 1))
    p1 = str(tmp_path / "pass1.sam")
    with open(p1, "w") as fh:
        fh.write("".join(sam))
    sf = str(tmp_path / "splices")
    rc, out, _ = run_cli(["junctions", "-x", generic["base"], "--junction-file", generic["src"], "-sf", sf, "-p1", p1, "-r", "4",
                          "-f", "bed"], stdin_text="not a query\n")
    assert rc == 0
    _, want_out, _ = run_cli(["search", "-x", generic["base"], "-f", "sam", "-r", "4"], stdin_text="".join(sam))
    from morna_amd.search import MornaSearch
    inv = {v: k for k, v in MornaSearch(generic["base"]).internal_id_map.items()}
    ref = ref_junctions(generic["lines"], [inv[i] for i in result_ids(want_out)], .05, 5, tables=generic["tables"])
    assert len(result_ids(want_out)) == 4
    assert out == want_out + "Number of retained junctions: %d\n" % ref["count"]
    assert read(sf) == ref["text"] and ref["count"] > 0


def test_stale_store_and_search_output(generic, tmp_path):
    """`index` without the flag removes the store of an earlier index of the same basename, and `junctions` then fails naming
    the flag; `search` prints the same with and without a store."""
    base = str(tmp_path / "idx")
    common = ["index", "--intropolis", generic["src"], "-x", base, "--features", "128", "--n-trees", "5", "-s", "10", "-t", "4"]
    assert run_cli(common + ["--junction-store"])[0] == 0
    assert os.path.exists(base + ".junc.mor")
    raw = "chr10\t100773221\t100780597\t3\nchr7\t1\t2\t5\n" + "".join(
        "%s\t%s\t%s\t2\n" % tuple(generic["lines"][j].split("\t")[:3]) for j in (10, 16, 19))
    with_store = [run_cli(["search", "-x", base, "-q", "3", "-r", "5", "-d"])[1],
                  run_cli(["search", "-x", base, "-f", "raw", "-r", "5", "-d", "-e"], raw)[1]]
    assert all(len(result_ids(t)) == 5 for t in with_store)
    with open(base + ".junc.mor", "rb") as fh:
        first = fh.read()
    with open(generic["base"] + ".junc.mor", "rb") as fh:
        assert fh.read() == first                                           # the same file indexed twice: the same bytes
    assert run_cli(common)[0] == 0
    assert not os.path.exists(base + ".junc.mor")
    without = [run_cli(["search", "-x", base, "-q", "3", "-r", "5", "-d"])[1],
               run_cli(["search", "-x", base, "-f", "raw", "-r", "5", "-d", "-e"], raw)[1]]
    assert without == with_store
    sf = str(tmp_path / "splices")
    with pytest.raises((IOError, RuntimeError), match="--junction-store"):
        run_cli(["junctions", "-x", base, "--junction-file", generic["src"], "-sf", sf, "-q", "3"])
    assert not os.path.exists(sf)
    from morna_amd.search import MornaSearch
    with pytest.raises((IOError, RuntimeError), match="--junction-store"):
        MornaSearch(base).retain_junctions([[0, 1]], .05, 5)


# ---- tiny_intropolis.tsv -------------------------------------------------------------------------------------------------
def test_tiny_store_and_one_query(tmp_path):
    from morna_amd.junctions import JunctionStore
    lines = tiny_lines()
    src, base = str(tmp_path / "tiny.tsv.gz"), str(tmp_path / "tiny")
    _write_gz(src, lines)
    assert run_cli(["index", "--intropolis", src, "-x", base, "--features", "128", "--n-trees", "4", "--junction-store"])[0] == 0
    tables = sample_lists(lines)
    juncs, covrs = tables
    store = JunctionStore.load(base + ".junc.mor")
    assert (store.n_samples, store.n_lines, store.nnz) == (6850, 3, sum(len(v) for v in juncs.values()))
    assert store.sample_ids().tolist() == list(juncs)
    for sample in juncs:
        line, cov = store.sample(sample)
        assert line.tolist() == juncs[sample] and cov.tolist() == [int(c) for c in covrs[sample]]
    ref, _ = check_single(base, lines, tables, src, tmp_path, ["-q", str(list(juncs)[17]), "-d"], ".05,5")
    assert ref["count"] == 3


# ---- the synthetic cohort (test_gpu_query_batch.py's shape) ----------------------------------------------------------------
@pytest.fixture(scope="module")
def cohort(tmp_path_factory):
    from morna_amd.synth import index_and_query_files
    d = tmp_path_factory.mktemp("jcohort")
    ipath, qpath = str(d / "index.tsv.gz"), str(d / "queries.tsv")
    ids = index_and_query_files(ipath, qpath, N_INDEX, N_QUERY, J=J)
    base = str(d / "idx")
    assert run_cli(["index", "--intropolis", ipath, "-x", base, "--features", str(DIM), "--n-trees", str(TREES), "-t", str(THRESHOLD),
                    "--junction-store"])[0] == 0
    with gzip.open(ipath, "rt") as fh:
        lines = fh.readlines()
    from morna_amd.search import MornaSearch
    s = MornaSearch(base)
    under = sum(1 for ln in lines if ln.split("\t")[6].count(",") + 1 < THRESHOLD)
    assert under > 500 and 0 < len(s.sample_frequencies) <= len(lines) - under      # lines the index drops and the store keeps
    return dict(dir=d, index=ipath, queries=qpath, ids=ids, base=base, lines=lines, tables=sample_lists(lines),
                inv={v: k for k, v in s.internal_id_map.items()}, indexed=sorted(s.internal_id_map))


def check_batch(cohort, base, tmp, query_flags, n_queries, filt=".05,5"):
    """One batch run: stdout is `search`'s and then one count per query, every <splicefile>.<sample id> the restatement's."""
    sf = str(tmp / "splices")
    rc, out, err = run_cli(["junctions", "-x", base, "--junction-file", cohort["index"], "-sf", sf, "--junction-filter", filt]
                           + query_flags)
    assert rc == 0
    _, want_out, _ = run_cli(["search", "-x", base] + query_flags)
    found = blocks(want_out)
    assert len(found) == n_queries
    counts, files = [], {}
    for sample, body in found:
        ref = ref_junctions(cohort["lines"], [cohort["inv"][i] for i in result_ids(body)], *parts_of(filt), tables=cohort["tables"])
        counts.append(ref["count"])
        files[sample] = read(sf + "." + str(sample))
        assert files[sample] == ref["text"], sample
    assert out == want_out + "".join("Number of retained junctions: %d\n" % n for n in counts)
    assert [ln for ln in err.split("\n") if ln.endswith("to begin with")] == ["%d junctions to begin with" % n for n in counts]
    assert sorted(os.listdir(str(tmp))) == sorted("splices.%d" % s for s, _ in found)
    assert min(counts) > 0 and len(set(counts)) > 1
    return out, files


def test_cohort_store_holds_every_line(cohort):
    from morna_amd.junctions import JunctionStore
    store = JunctionStore.load(cohort["base"] + ".junc.mor")
    juncs, covrs = cohort["tables"]
    assert (store.n_samples, store.n_lines, store.nnz) == (len(juncs), len(cohort["lines"]), sum(len(v) for v in juncs.values()))
    assert store.sample_ids().tolist() == list(juncs)
    assert store.n_samples > len(cohort["indexed"]) - 1                     # samples seen only under the threshold included
    for sample in juncs:
        line, cov = store.sample(sample)
        assert line.tolist() == juncs[sample] and cov.tolist() == [int(c) for c in covrs[sample]]


def test_cohort_batch_query_ids(cohort, tmp_path):
    picks = cohort["indexed"][::len(cohort["indexed"]) // 64][:64]
    assert len(picks) == 64
    check_batch(cohort, cohort["base"], tmp_path, ["--query-ids", ",".join(map(str, picks)), "-d"], 64)


def test_cohort_batch_intropolis_approximate(cohort, tmp_path):
    check_batch(cohort, cohort["base"], tmp_path, ["--intropolis", cohort["queries"]], N_QUERY, filt=".5,40")


def test_cohort_batch_intropolis_exact_and_two_shards(cohort, tmp_path, monkeypatch):
    """-e, and the same files from an index of two row shards loaded by one process (one global store); one process per
    shard is refused with the batch search's wording."""
    (tmp_path / "one").mkdir()
    (tmp_path / "two").mkdir()
    flags = ["--intropolis", cohort["queries"], "-e", "-d"]
    out1, files1 = check_batch(cohort, cohort["base"], tmp_path / "one", flags, N_QUERY)
    base2 = str(cohort["dir"] / "idx2")
    assert run_cli(["index", "--intropolis", cohort["index"], "-x", base2, "--features", str(DIM), "--n-trees", str(TREES),
                    "-t", str(THRESHOLD), "--shards", "2", "--junction-store"])[0] == 0
    assert os.path.exists(base2 + ".shards.mor")
    with open(base2 + ".junc.mor", "rb") as f2, open(cohort["base"] + ".junc.mor", "rb") as f1:
        assert f1.read() == f2.read()
    out2, files2 = check_batch(cohort, base2, tmp_path / "two", flags, N_QUERY)
    assert out1 == out2 and files1 == files2
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setenv("RANK", "0")
    with pytest.raises(RuntimeError, match="not available with one process per shard"):
        run_cli(["junctions", "-x", base2, "--junction-file", cohort["index"], "-sf", str(tmp_path / "refused")] + flags)


@pytest.mark.parametrize("r", [1, 20, 64])
def test_cohort_result_counts(cohort, tmp_path, r):
    sample = cohort["indexed"][123]
    ref, results = check_single(cohort["base"], cohort["lines"], cohort["tables"], cohort["index"], tmp_path,
                                ["-q", str(sample), "-r", str(r), "--search-k", "2000"], ".05,5")
    assert len(results) == r and ref["count"] > 0


def test_cohort_65_results_is_a_value_error(cohort, tmp_path):
    sf = str(tmp_path / "splices")
    with pytest.raises(ValueError, match="64"):
        run_cli(["junctions", "-x", cohort["base"], "--junction-file", cohort["index"], "-sf", sf, "-q",
                 str(cohort["indexed"][0]), "-r", "65"])
    assert not os.path.exists(sf)
    from morna_amd.search import MornaSearch
    with pytest.raises(ValueError, match="64"):
        MornaSearch(cohort["base"]).retain_junctions([list(range(65))], .05, 5)


# ---- determinism ---------------------------------------------------------------------------------------------------------
def test_store_build_is_deterministic(cohort, tmp_path):
    """Two builds: the same bytes.  Every line's sample list reversed: the same content per sample."""
    from morna_amd.index import ParsedLines
    from morna_amd.junctions import JunctionStore
    blobs = []
    for n in range(2):
        store = JunctionStore.build(ParsedLines(cohort["index"], sample_count=1, sample_threshold=0))
        path = str(tmp_path / ("s%d.junc.mor" % n))
        store.save(path)
        with open(path, "rb") as fh:
            blobs.append(fh.read())
    with open(cohort["base"] + ".junc.mor", "rb") as fh:
        assert blobs[0] == blobs[1] == fh.read()
    assert store.timers()["build"][0] > 0 and store.timers()["build"][1] == 16 * store.nnz
    rev = []
    for ln in cohort["lines"]:
        t = ln.rstrip("\n").split("\t")
        rev.append("\t".join(t[:6] + [",".join(reversed(t[6].split(","))), ",".join(reversed(t[7].split(",")))]) + "\n")
    rpath = str(tmp_path / "reversed.tsv.gz")
    _write_gz(rpath, rev)
    other = JunctionStore.build(ParsedLines(rpath, sample_count=1, sample_threshold=0))
    assert sorted(other.sample_ids().tolist()) == sorted(store.sample_ids().tolist())
    assert other.sample_ids().tolist() != store.sample_ids().tolist()       # first-seen order differs
    for sample in store.sample_ids().tolist():
        a, b = store.sample(sample), other.sample(sample)
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


def test_store_build_rejects_bad_input(tmp_path, embedded):
    from morna_amd.index import ParsedLines
    from morna_amd.junctions import JunctionStore
    lines = list(embedded["generic"])
    t = lines[13].rstrip("\n").split("\t")
    first = t[6].split(",")[0]
    lines[13] = "\t".join(t[:6] + [t[6] + "," + first, t[7] + ",9"]) + "\n"
    src = str(tmp_path / "twice.gz")
    _write_gz(src, lines)
    with pytest.raises(ValueError, match=r"line 13 lists sample %s twice" % first):
        JunctionStore.build(ParsedLines(src, sample_count=10, sample_threshold=0))
    good = str(tmp_path / "good.gz")
    _write_gz(good, embedded["generic"])
    with pytest.raises(ValueError, match="threshold 0"):                    # lines dropped: kept line j is not file line j
        JunctionStore.build(ParsedLines(good, sample_count=10, sample_threshold=4))


# ---- the filter's written output at the tile edges ---------------------------------------------------------------------------
def test_retained_output_equals_restatement_at_the_tile_edges():
    """lines, found_in and coverages of `retain` against ref_retain on the stores of test_gpu_recovery: one tile, both
    sides of the tile edge, three tiles and a remainder, with lines 4095 and 4096 held by every seventh sample.  Recovery
    and the filter walk a tile with the same code, so that recovery agrees with the filter there pins neither."""
    from test_gpu_recovery import SIZES, make_store            # (that module imports this one)
    for n_lines in SIZES:
        case = make_store(n_lines)
        store, rows, lists = case["store"], case["rows"], case["lists"]
        cov_at = {s: dict(zip(line.tolist(), cov.tolist())) for s, (line, cov) in rows.items()}
        for f, c in [(0.0, 10**6), (0.5, 3), (1.0, 1)]:
            kept = store.retain(lists, f, c)
            assert len(kept) == len(lists)
            seen = set()
            for q, lst in enumerate(lists):
                retained, found_in = ref_retain([rows[s][0].tolist() for s in lst], [rows[s][1].tolist() for s in lst], f, c)
                lines = sorted(retained)
                assert kept[q].lines.tolist() == lines, (n_lines, f, c, q)
                assert kept[q].found_in == [found_in[j] for j in lines], (n_lines, f, c, q)
                assert kept[q].coverages == [[cov_at[lst[r]][j] for r in found_in[j]] for j in lines], (n_lines, f, c, q)
                seen.update(lines)
            if n_lines > 4096 and (f, c) == (0.0, 10**6):
                assert 4095 in seen and 4096 in seen
