"""Depth thinning on the GPU: `JunctionStore.thin` against its numpy restatement (test_thin_cpu.ref_thin)
entry for entry on synthetic stores with rows at the edges of a chunk and coverages at the edges of the kernel's two draw
loops; and the command line -- `search --downsample` blocks against those `search --intropolis` prints for a file that
holds the thinned coverages, `recovery --downsample` tables against the set-and-dict restatement fed the lists the search
printed.  Integers and whole text.  -m gpu"""
import gzip
import os
import re
import subprocess

import numpy as np
import pytest

from test_gpu_junctions import _write_gz, blocks, result_ids, run_cli
from test_gpu_recovery import summary_text, table_text
from test_junctions_cpu import ref_retain, sample_lists
from test_pool_cpu import ref_pool
from test_recovery_cpu import ref_hist, ref_recovery, rows_of_tables
from test_thin_cpu import (CHUNK, DEEPEST, EMPTY, FIRST_ID, N_SAMPLES, NEGATIVE, PLANTED_IN, SIZES, THRESHOLDS, TOO_DEEP, ZERO_STATS,
                           check_refusals, good_ids, make_rows, ref_thin)

pytestmark = pytest.mark.gpu

SEEDS = [8675309, 1]


def make_store(n_lines):
    """The rows of test_thin_cpu.make_rows as a store, with the restatement's answer for every good sample, threshold and
    seed, computed once."""
    from morna_amd.junctions import JunctionStore
    rows = make_rows(n_lines)
    ext = np.arange(FIRST_ID, FIRST_ID + N_SAMPLES, dtype=np.int64)
    ptr = np.zeros(N_SAMPLES + 1, np.int64)
    ptr[1:] = np.cumsum([len(rows[s][0]) for s in ext.tolist()])
    store = JunctionStore.from_arrays(ext, ptr, np.concatenate([rows[s][0] for s in ext.tolist()]),
                                      np.concatenate([rows[s][1] for s in ext.tolist()]), n_lines)
    ids = good_ids(rows)
    want = {}
    for seed in SEEDS:
        for s in ids:
            cache = {}
            for a in THRESHOLDS:
                want[(s, a, seed)] = ref_thin(rows, s, a, seed, cache)
    return dict(store=store, rows=rows, n_lines=n_lines, ids=ids, want=want)


@pytest.fixture(scope="module", params=SIZES)
def case(request):
    return make_store(request.param)


def same(got, want):
    return (got.lines.dtype, got.cov.dtype) == (np.int32, np.int32) and len(got) == len(want[0]) \
        and np.array_equal(got.lines, want[0]) and np.array_equal(got.cov, want[1])


def chunks_of(case, ids):
    return sum((len(case["rows"][s][0]) + CHUNK - 1) // CHUNK for s in ids)


def test_thin_equals_restatement_and_nests(case):
    store, rows, ids, want, n = case["store"], case["rows"], case["ids"], case["want"], case["n_lines"]
    assert len(ids) == N_SAMPLES - 2 and [len(rows[s][0]) for s in (1045, 1046, 1047, 1048)] == \
        [min(m, n) for m in (CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 7)]
    if n == SIZES[-1]:
        assert {0, 1, 31, 32, 33, 64, 65, 4096, 100000, 2**24} <= set(rows[DEEPEST][1].tolist())
        assert all(0 in rows[s][1] for s in PLANTED_IN)
    entries, draws = sum(len(rows[s][0]) for s in ids), sum(int(rows[s][1].sum()) for s in ids)
    for seed in SEEDS:
        before = [np.zeros(n, np.int64) for _ in ids]
        for a in sorted(THRESHOLDS):
            got = store.thin(ids, a, seed)
            assert len(got) == len(ids)
            for q, s in enumerate(ids):
                assert same(got[q], want[(s, a, seed)]), (n, s, a, seed)
                now = np.zeros(n, np.int64)
                now[got[q].lines] = got[q].cov
                assert (now >= before[q]).all(), (n, s, a, seed)          # the thresholds nest, on the GPU's own output
                before[q] = now
            stats = store.thin_stats()
            survivors = sum(len(r) for r in got)
            assert stats["draws"] == draws and stats["bytes_read"] == 16 * entries
            assert stats["bytes_written"] == 4 * entries + 8 * survivors
            assert stats["workgroups"] == chunks_of(case, ids) and stats["kernel_ms"] > 0
            assert len(got[ids.index(EMPTY)]) == 0
            if a == 0:
                assert survivors == 0
            if a == 2**32:
                assert survivors == sum(int((rows[s][1] > 0).sum()) for s in ids)
    assert any(want[(s, 2**31, 1)][1].tolist() != want[(s, 2**31, 8675309)][1].tolist() for s in ids)
    assert store.thin([], [], 5) == [] and store.thin_stats() == ZERO_STATS


def test_thin_does_not_depend_on_the_batch(case):
    store, ids, want = case["store"], case["ids"], case["want"]
    s, other = 1048, 1020
    a = 429496730
    one = store.thin([s], a, 1)
    three = store.thin([other, s, EMPTY], a, 1)
    many = store.thin([s] * 64 + [other], a, 1)
    assert same(one[0], want[(s, a, 1)]) and same(three[1], want[(s, a, 1)]) and same(three[0], want[(other, a, 1)])
    assert len(three[2]) == 0 and all(same(many[q], want[(s, a, 1)]) for q in range(64)) and same(many[64], want[(other, a, 1)])
    assert one[0].lines.tobytes() == three[1].lines.tobytes() == many[63].lines.tobytes()
    assert one[0].cov.tobytes() == three[1].cov.tobytes() == many[63].cov.tobytes()
    # the same id at every threshold in one batch, among others
    jobs = [(s, t) for t in THRESHOLDS] + [(other, 2**31), (1047, 1), (s, 2**31)]
    got = store.thin([j[0] for j in jobs], [j[1] for j in jobs], 8675309)
    for q, (i, t) in enumerate(jobs):
        assert same(got[q], want[(i, t, 8675309)]), (case["n_lines"], i, t)
    again = store.thin([j[0] for j in jobs], [j[1] for j in jobs], 8675309)        # two calls: identical bytes
    for x, y in zip(got, again):
        assert x.lines.tobytes() == y.lines.tobytes() and x.cov.tobytes() == y.cov.tobytes()
    assert store.thin_stats()["workgroups"] == chunks_of(case, [j[0] for j in jobs])


def test_refusals_leave_the_store_and_its_siblings_as_they_were():
    case = make_store(2049)
    store, rows, n = case["store"], case["rows"], case["n_lines"]
    lists = [case["ids"][:64], case["ids"][70:90], [1000, 1001], []]
    groups = [case["ids"][:70], [1002], []]
    grid = [1, 2, 3, 5, 10, 20, 50, 1000]
    truths = [rows[1005][0], [], np.arange(n), [0]]

    def siblings():
        kept = store.retain(lists, 0.5, 3)
        hist = store.recovery(lists, truths, grid)
        pooled = store.pool(groups)
        return kept, hist, pooled, store.timers()["retain"], store.recovery_stats(), store.pool_stats()
    before = siblings()
    assert before[3][0] > 0 and before[4]["kernel_ms"] > 0 and before[5]["kernel_ms"] > 0
    at = {s: int(rows[s][0][len(rows[s][0]) // 2]) for s in (NEGATIVE, TOO_DEEP)}
    check_refusals(store, 1000, NEGATIVE, TOO_DEEP, at[NEGATIVE], at[TOO_DEEP])
    got = store.thin([1000, 1048], 2**31, 1)                     # and it thins afterwards
    assert same(got[0], case["want"][(1000, 2**31, 1)]) and same(got[1], case["want"][(1048, 2**31, 1)])
    assert store.thin_stats()["kernel_ms"] > 0
    assert (store.timers()["retain"], store.recovery_stats(), store.pool_stats()) == before[3:]      # their timers stay their own
    after = siblings()
    for q, lst in enumerate(lists):
        retained, _ = ref_retain([rows[s][0].tolist() for s in lst], [rows[s][1].tolist() for s in lst], 0.5, 3)
        assert after[0][q].lines.tolist() == sorted(retained) == before[0][q].lines.tolist()
        assert after[0][q].masks.tobytes() == before[0][q].masks.tobytes() and after[0][q].coverages == before[0][q].coverages
    assert np.array_equal(after[1], before[1])
    assert np.array_equal(after[1], np.stack([ref_hist(rows, n, lst, t, grid) for lst, t in zip(lists, truths)]))
    for g, (x, y) in enumerate(zip(after[2], before[2])):
        want = ref_pool(rows, n, groups[g])
        assert np.array_equal(x.lines, want[0]) and np.array_equal(x.sums, want[1]) and x.sums.tobytes() == y.sums.tobytes()
    assert store.thin_stats()["kernel_ms"] > 0                    # and thin's own stay through theirs


def test_c_program_against_the_header_alone(tmp_path):
    """tests/c/thin_caller.c, compiled with gcc against include/morna_hip.h alone, run as a process of its own."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe, libdir = str(tmp_path / "thin_caller"), os.path.join(root, "morna_amd")
    subprocess.check_call(["gcc", "-O1", "-Wall", "-Werror", "-std=c99", "-I", os.path.join(root, "include"),
                           os.path.join(root, "tests", "c", "thin_caller.c"), "-o", exe, "-L", libdir, "-lmorna_hip",
                           "-Wl,-rpath," + libdir, "-lm"])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "thin caller ok" in r.stdout


# ---- the command line on a synthetic cohort --------------------------------------------------------------------------------------
N_INDEX, N_QUERY, J, THRESHOLD, TREES, DIM = 600, 40, 3000, 30, 5, 128
RATES, KEEP = ["0.5", "0.1"], [2**31, 429496730]
SEED = 8675309


def thin_blocks(text):
    parts = re.split(r"^# query (-?\d+)\tkeep (\S+)\n", text, flags=re.M)
    assert parts[0] == ""
    return [((int(parts[i]), parts[i + 1]), parts[i + 2]) for i in range(1, len(parts), 3)]


@pytest.fixture(scope="module")
def cohort(tmp_path_factory):
    from morna_amd.search import MornaSearch
    from morna_amd.synth import index_and_query_files
    d = tmp_path_factory.mktemp("thin_cohort")
    ipath = str(d / "index.tsv.gz")
    index_and_query_files(ipath, str(d / "unused.tsv"), N_INDEX, N_QUERY, J=J)
    base, meta = str(d / "idx"), str(d / "meta.tsv")
    with gzip.open(ipath, "rt") as fh:
        lines = fh.readlines()
    tables = sample_lists(lines)
    rows = rows_of_tables(tables)
    ids = sorted(rows)
    with open(meta, "w") as fh:
        fh.write("".join("%d\tsample%d tissue%d\n" % (s, s, s % 7) for s in ids))
    assert run_cli(["index", "--intropolis", ipath, "-x", base, "--features", str(DIM), "--n-trees", str(TREES), "-t", str(THRESHOLD),
                    "-m", meta, "--junction-store"])[0] == 0
    queries = [ids[5], ids[311], ids[77]]                      # not in ascending order: the blocks follow the order given
    jobs = [(s, rate) for s in queries for rate in RATES]
    thinned = {(s, rate): ref_thin(rows, s, a, SEED) for s in queries for rate, a in zip(RATES, KEEP)}
    assert all(len(t[0]) > 0 for t in thinned.values())
    # every (sample, rate) as a sample of its own in an intropolis file, with the thinned coverages
    label = {job: 9001 + k for k, job in enumerate(jobs)}
    by_line = {}
    for job in jobs:
        for j, c in zip(thinned[job][0].tolist(), thinned[job][1].tolist()):
            by_line.setdefault(j, []).append((label[job], c))
    thinned_file = str(d / "thinned.tsv.gz")
    _write_gz(thinned_file, ["\t".join(lines[j].split("\t")[:6] + [",".join(str(s) for s, _ in by_line[j]),
                                                                     ",".join(str(c) for _, c in by_line[j])]) + "\n"
                             for j in sorted(by_line)])
    inv = {v: k for k, v in MornaSearch(base).internal_id_map.items()}
    return dict(dir=d, index=ipath, base=base, lines=lines, tables=tables, rows=rows, queries=queries, jobs=jobs, thinned=thinned,
                label=label, thinned_file=thinned_file, inv=inv)


def downsample_flags(cohort):
    return ["--query-ids", ",".join(map(str, cohort["queries"])), "--downsample", ",".join(RATES), "--junction-file", cohort["index"]]


@pytest.mark.parametrize("mode", [[], ["-e"], ["--unhashed"], ["-m"], ["-e", "-m"]])
def test_search_downsample_equals_search_of_the_thinned_file(cohort, mode):
    rc, got, _ = run_cli(["search", "-x", cohort["base"], "-d", "-r", "10"] + downsample_flags(cohort) + mode)
    assert rc == 0
    rc, want, _ = run_cli(["search", "-x", cohort["base"], "--intropolis", cohort["thinned_file"], "--junction-file", cohort["index"],
                           "-d", "-r", "10"] + mode)
    assert rc == 0
    got_blocks, want_blocks = thin_blocks(got), dict(blocks(want))
    assert [job for job, _ in got_blocks] == cohort["jobs"]                # the ids in the order given, the rates as typed
    assert sorted(want_blocks) == sorted(cohort["label"].values())
    for job, body in got_blocks:
        assert body == want_blocks[cohort["label"][job]], (mode, job)
        assert len(result_ids(body)) == 10
        assert ("tissue" in body) == ("-m" in mode)
    assert len(set(body for _, body in got_blocks)) > 1
    if not mode:                                                # another seed keeps other reads: other blocks
        rc, other, _ = run_cli(["search", "-x", cohort["base"], "-d", "-r", "10", "--downsample-seed", "2"] + downsample_flags(cohort))
        assert rc == 0 and [job for job, _ in thin_blocks(other)] == cohort["jobs"] and other != got
        with pytest.raises(ValueError, match="424242"):
            run_cli(["search", "-x", cohort["base"], "-q", "424242", "--downsample", "0.5", "--junction-file", cohort["index"]])


@pytest.mark.parametrize("mode", [[], ["-e"]])
@pytest.mark.parametrize("lost", [[], ["--lost-only"]])
def test_recovery_downsample_equals_restatement(cohort, mode, lost):
    from morna_amd.junctions import format_recovery_rows, parse_recovery_grid, sum_recovery_rows
    frequencies, coverages = parse_recovery_grid()
    r = 5
    rc, out, _ = run_cli(["recovery", "-x", cohort["base"], "-r", str(r)] + downsample_flags(cohort) + mode + lost)
    assert rc == 0
    rc, searched, _ = run_cli(["search", "-x", cohort["base"], "-r", str(r + 1)] + downsample_flags(cohort) + mode)
    assert rc == 0
    found = thin_blocks(searched)
    assert [job for job, _ in found] == cohort["jobs"]
    texts, tables = [], {rate: [] for rate in RATES}
    for (s, rate), body in found:
        results = [cohort["inv"][i] for i in result_ids(body) if cohort["inv"][i] != s][:r]
        assert len(results) == r
        line, cov = cohort["rows"][s]
        truth = line[cov >= 1].tolist()
        if lost:
            truth = sorted(set(truth) - set(cohort["thinned"][(s, rate)][0].tolist()))
            assert 0 < len(truth) < len(line) or rate != "0.1"
        text, rows = table_text(cohort["rows"], len(cohort["lines"]), s, results, truth, 0, frequencies, coverages)
        at = 0
        for f in frequencies:                                  # the rows against the set-and-dict restatement itself
            for c in coverages:
                retrieved, tp, true = ref_recovery(cohort["lines"], results, truth, float(f), c, cohort["tables"])
                assert (rows[at]["retrieved"], rows[at]["true_positive"], rows[at]["false_negative"]) == (retrieved, tp, true - tp)
                at += 1
        head, rest = text.split("\n", 1)
        assert head == "# query %d\tresults %d\ttrue %d" % (s, r, len(truth))
        texts.append("# query %d\tkeep %s\tresults %d\ttrue %d\n" % (s, rate, r, len(truth)) + rest)
        tables[rate].append(rows)
    summaries = "".join("# all %d queries\tkeep %s\n" % (len(cohort["queries"]), rate) + format_recovery_rows(sum_recovery_rows(tables[rate]))
                        for rate in RATES)
    assert out == "".join(texts) + summaries
    rc, only, _ = run_cli(["recovery", "-x", cohort["base"], "-r", str(r), "--summary-only"] + downsample_flags(cohort) + mode + lost)
    assert rc == 0 and only == summaries


def test_a_job_that_keeps_no_read_is_named_on_stderr(cohort):
    """Rate 0 keeps nothing: the job is searched as a sample without junctions, and both commands say so.  The other jobs are
    as without it."""
    flags = ["--query-ids", ",".join(map(str, cohort["queries"])), "--junction-file", cohort["index"], "-e", "-r", "5"]
    notes = "".join("query %d at keep 0 keeps no read: it is searched as a sample without junctions\n" % s for s in cohort["queries"])
    rc, searched, err = run_cli(["search", "-x", cohort["base"], "--downsample", "0.5,0"] + flags)
    found = thin_blocks(searched)
    assert rc == 0 and err == notes
    assert [job for job, _ in found] == [(s, rate) for s in cohort["queries"] for rate in ("0.5", "0")]
    rc, half, err = run_cli(["search", "-x", cohort["base"], "--downsample", "0.5"] + flags)
    assert rc == 0 and err == "" and thin_blocks(half) == [blk for blk in found if blk[0][1] == "0.5"]
    rc, out, err = run_cli(["recovery", "-x", cohort["base"], "--downsample", "0.5,0"] + flags)
    assert rc == 0 and err == notes
    rc, alone, err = run_cli(["recovery", "-x", cohort["base"], "--downsample", "0.5"] + flags)
    assert rc == 0 and err == "" and alone.split("# all")[0] == "".join(
        block for block in re.split(r"(?=^# query )", out.split("# all")[0], flags=re.M) if "\tkeep 0.5\t" in block)


def test_recovery_without_downsample_prints_what_it_printed(cohort):
    """The path --downsample does not take: the tables test_gpu_recovery's restatement builds for a leave-one-out run."""
    from morna_amd.junctions import parse_recovery_grid
    frequencies, coverages = parse_recovery_grid()
    flags = ["--query-ids", ",".join(map(str, cohort["queries"]))]
    rc, out, _ = run_cli(["recovery", "-x", cohort["base"], "-r", "5"] + flags)
    assert rc == 0
    _, searched, _ = run_cli(["search", "-x", cohort["base"], "-r", "6"] + flags)
    texts, tables = [], []
    for s, body in blocks(searched):
        results = [cohort["inv"][i] for i in result_ids(body) if cohort["inv"][i] != s][:5]
        line, cov = cohort["rows"][s]
        text, rows = table_text(cohort["rows"], len(cohort["lines"]), s, results, line[cov >= 1].tolist(), 0, frequencies, coverages)
        texts.append(text)
        tables.append(rows)
    assert len(texts) == 3 and out == "".join(texts) + summary_text(tables)
