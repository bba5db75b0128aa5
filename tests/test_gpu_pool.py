"""Pooled samples on the GPU: `JunctionStore.pool` against its numpy restatement (test_pool_cpu.ref_pool)
entry for entry on synthetic stores at the tile edges and with groups at the edges of a round of 64 members; and the
command line -- `supersample` files against the restatement of create_supersample.py byte for byte, `search --supersamples`
blocks against those `search --intropolis` prints for a file that holds the same sums.  Integers and whole text.  -m gpu
Stores of more than 64 tiles, where rounds of 64 members meet rounds of 64 tiles: test_gpu_jstore_many_tiles.py."""
import gzip

import numpy as np
import pytest

from test_gpu_junctions import _write_gz, blocks, read, run_cli
from test_junctions_cpu import ref_retain, sample_lists
from test_pool_cpu import ZERO_STATS, ref_pool, ref_supersample
from test_recovery_cpu import ref_hist, rows_of_tables

pytestmark = pytest.mark.gpu

N_SAMPLES, EMPTY, BIG = 200, 1040, 2**31 - 1   # external ids 1000 .. 1199; 1040 holds no line
SIZES = [1, 4095, 4096, 4097, 12290]           # one tile, both sides of the tile edge, three tiles and a remainder
GROUP_SIZES = [1, 2, 63, 64, 65, 128, 129, 200]   # both sides of a round's edge, two full rounds, a remainder, the whole store


def make_store(n_lines):
    """200 samples over n_lines lines at about 5 % density, coverages 1 + geometric.  Sample 1040 is empty.  Line 0 is held
    by 1000 at -7 and by 1001 at +7 (sum 0, holders 2) and by nobody else; every seventh sample holds lines 4095, 4096 and
    the last one; 1002, 1003 and 1004 hold line min(4096, n_lines - 1) at 2^31 - 1 each."""
    from morna_amd.junctions import JunctionStore
    rng = np.random.Generator(np.random.PCG64(20268 + n_lines))
    ext = np.arange(1000, 1000 + N_SAMPLES, dtype=np.int64)
    big_line = min(4096, n_lines - 1)
    rows = {}
    for i, s in enumerate(ext.tolist()):
        held = rng.random(n_lines) < 0.05
        if i % 7 == 0:
            held[[j for j in (4095, 4096, n_lines - 1) if j < n_lines]] = True
        held[0] = i in (0, 1)
        if i in (2, 3, 4):
            held[big_line] = True
        if s == EMPTY:
            held[:] = False
        line = np.nonzero(held)[0].astype(np.int64)
        cov = rng.geometric(0.2, len(line)).astype(np.int64)
        if i in (0, 1):
            cov[0] = -7 if i == 0 else 7
        if i in (2, 3, 4):
            cov[line == big_line] = BIG
        rows[s] = (line, cov)
    ptr = np.zeros(N_SAMPLES + 1, np.int64)
    ptr[1:] = np.cumsum([len(rows[s][0]) for s in ext.tolist()])
    store = JunctionStore.from_arrays(ext, ptr, np.concatenate([rows[s][0] for s in ext.tolist()]),
                                      np.concatenate([rows[s][1] for s in ext.tolist()]), n_lines)
    groups = [[], [EMPTY], [1002], [1000, 1001]] + [rng.permutation(ext)[:m].tolist() for m in GROUP_SIZES[2:]]
    groups.append(rng.permutation(groups[8]).tolist())          # the 129 in another order
    want = [ref_pool(rows, n_lines, g) for g in groups]
    return dict(store=store, rows=rows, n_lines=n_lines, ext=ext, groups=groups, want=want, big_line=big_line)


@pytest.fixture(scope="module", params=SIZES)
def case(request):
    return make_store(request.param)


def same(got, want):
    return (got.lines.dtype, got.sums.dtype, got.holders.dtype) == (np.int32, np.int64, np.int32) and len(got) == len(want[0]) \
        and np.array_equal(got.lines, want[0]) and np.array_equal(got.sums, want[1]) and np.array_equal(got.holders, want[2])


def test_pool_equals_restatement(case):
    store, groups, want, n = case["store"], case["groups"], case["want"], case["n_lines"]
    assert [len(g) for g in groups[2:10]] == GROUP_SIZES
    got = store.pool(groups)
    assert len(got) == len(groups)
    for g in range(len(groups)):
        assert same(got[g], want[g]), (n, g)
    assert len(got[0]) == 0 and len(got[1]) == 0
    assert (got[3].lines[0], got[3].sums[0], got[3].holders[0]) == (0, 0, 2)          # -7 and +7: held, whatever the sum
    at = int(np.searchsorted(got[9].lines, case["big_line"]))
    assert got[9].lines[at] == case["big_line"] and got[9].sums[at] >= 3 * BIG - 7 > 2**32 and got[9].holders[at] >= 3
    if n > 4096:
        assert {0, 4095, 4096, n - 1} <= set(got[9].lines.tolist())
    assert same(got[10], want[8]) and sorted(groups[10]) == sorted(groups[8]) and groups[10] != groups[8]
    entries = sum(len(case["rows"][s][0]) for g in groups for s in g)
    stats = store.pool_stats()
    assert stats["bytes_read"] == 2 * 8 * entries and stats["bytes_written"] == 16 * sum(len(w[0]) for w in want)
    assert stats["workgroups"] == len(groups) * ((n + 4095) // 4096) and stats["kernel_ms"] > 0
    again = store.pool(groups)                                   # two calls: identical arrays
    for a, b in zip(got, again):
        assert a.lines.tobytes() == b.lines.tobytes() and a.sums.tobytes() == b.sums.tobytes() \
            and a.holders.tobytes() == b.holders.tobytes()
    assert store.pool([]) == [] and store.pool_stats() == ZERO_STATS
    assert same(store.pool([[1003, 1003, 1002, 1003]])[0], ref_pool(case["rows"], n, [1003, 1002]))   # repeats count once


def test_pool_does_not_depend_on_the_batch(case):
    store, groups, want = case["store"], case["groups"], case["want"]
    g, other = groups[6], groups[9]                              # 65 members; the whole store
    one = store.pool([g])
    three = store.pool([other, g, []])
    many = store.pool([g] * 64 + [other])
    assert same(one[0], want[6]) and same(three[1], want[6]) and same(three[0], want[9]) and len(three[2]) == 0
    assert all(same(many[q], want[6]) for q in range(64)) and same(many[64], want[9])


def test_filter_and_recovery_after_pool_keep_their_answers_and_timers(case):
    store, rows, n = case["store"], case["rows"], case["n_lines"]
    lists = [case["groups"][5][:64], case["groups"][4][:20], [1000, 1001], []]
    before = store.retain(lists, 0.5, 3)
    retain_timers = store.timers()["retain"]
    assert retain_timers[0] > 0
    store.pool(case["groups"])
    assert store.timers()["retain"] == retain_timers            # the filter's slots stay its own
    kept = store.retain(lists, 0.5, 3)
    for q, lst in enumerate(lists):
        retained, _ = ref_retain([rows[s][0].tolist() for s in lst], [rows[s][1].tolist() for s in lst], 0.5, 3)
        assert kept[q].lines.tolist() == sorted(retained) == before[q].lines.tolist(), (n, q)
        assert kept[q].masks.tobytes() == before[q].masks.tobytes() and kept[q].coverages == before[q].coverages
    grid = [1, 2, 3, 5, 10, 20, 50, 1000]
    truths = [rows[1005][0], [], np.arange(n), [0]]
    hist = store.recovery(lists, truths, grid)
    assert np.array_equal(hist, np.stack([ref_hist(rows, n, lst, t, grid) for lst, t in zip(lists, truths)]))
    pool_stats = store.pool_stats()
    assert pool_stats["kernel_ms"] > 0 and pool_stats["workgroups"] == len(case["groups"]) * ((n + 4095) // 4096)


# ---- the command line on a synthetic cohort --------------------------------------------------------------------------------------
N_INDEX, N_QUERY, J, THRESHOLD, TREES, DIM = 600, 40, 3000, 30, 5, 128
LABELS = ["9001", "9002", "9003"]


@pytest.fixture(scope="module")
def cohort(tmp_path_factory):
    from morna_amd.synth import index_and_query_files
    d = tmp_path_factory.mktemp("pool_cohort")
    ipath = str(d / "index.tsv.gz")
    index_and_query_files(ipath, str(d / "unused.tsv"), N_INDEX, N_QUERY, J=J)
    base = str(d / "idx")
    assert run_cli(["index", "--intropolis", ipath, "-x", base, "--features", str(DIM), "--n-trees", str(TREES), "-t", str(THRESHOLD),
                    "--junction-store"])[0] == 0
    with gzip.open(ipath, "rt") as fh:
        lines = fh.readlines()
    under = sum(1 for ln in lines if ln.split("\t")[6].count(",") + 1 < THRESHOLD)
    assert 0 < under < len(lines)                               # lines the index drops and the store keeps
    tables = sample_lists(lines)
    rows = rows_of_tables(tables)
    ids = sorted(rows)
    rng = np.random.Generator(np.random.PCG64(88))
    groups = [rng.permutation(ids)[:m].tolist() for m in (100, 5, 20)]      # one of more than 64 members
    gpath = str(d / "groups.tsv")
    with open(gpath, "w") as fh:
        fh.write("".join("%s\t%s\n" % (label, ",".join(map(str, g))) for label, g in zip(LABELS, groups)))
    want = [ref_pool(rows, len(lines), g) for g in groups]
    # the groups as the samples of an intropolis file: the sums as coverages, the lines no group holds left out
    by_line = {}
    for label, (held, sums, _) in zip(LABELS, want):
        for j, c in zip(held.tolist(), sums.tolist()):
            by_line.setdefault(j, []).append((label, c))
    pooled_file = str(d / "pooled.tsv.gz")
    _write_gz(pooled_file, ["\t".join(lines[j].split("\t")[:6] + [",".join(s for s, _ in by_line[j]), ",".join(str(c) for _, c in by_line[j])])
                            + "\n" for j in sorted(by_line)])
    assert 0 < len(by_line) < len(lines)
    return dict(dir=d, index=ipath, base=base, lines=lines, rows=rows, groups=groups, gpath=gpath, want=want, pooled_file=pooled_file)


def group_line(label, group, want):
    return "# group %s\tsamples %d\tjunctions %d\tcoverage %d\n" % (label, len(group), len(want[0]), int(want[1].sum()))


def test_supersample_sample_ids_equals_create_supersample(cohort, tmp_path):
    group, want = cohort["groups"][0], cohort["want"][0]
    ids_file, out = str(tmp_path / "ids.txt"), str(tmp_path / "supersample.qry")
    with open(ids_file, "w") as fh:
        fh.write("".join("%d\n" % s for s in group[:50]) + "\n" + "".join("%d\n" % s for s in group[50:]))
    rc, stdout, _ = run_cli(["supersample", "-x", cohort["base"], "--sample-ids", ids_file, "--junction-file", cohort["index"], "-o", out])
    assert rc == 0 and stdout == group_line("supersample", group, want)
    text = read(out)
    assert text == ref_supersample(cohort["lines"], set(group))
    assert len(text.splitlines()) == len(cohort["lines"]) and 0 < len(want[0]) < len(cohort["lines"])
    with open(ids_file, "a") as fh:
        fh.write("424242\n")
    with pytest.raises(IndexError, match="424242"):            # the reference sums nothing for it; here it is an error
        run_cli(["supersample", "-x", cohort["base"], "--sample-ids", ids_file, "--junction-file", cohort["index"], "-o", out])


def test_supersample_groups_equals_create_supersample(cohort, tmp_path):
    out = str(tmp_path / "pooled")
    rc, stdout, _ = run_cli(["supersample", "-x", cohort["base"], "--groups", cohort["gpath"], "--junction-file", cohort["index"], "-o", out])
    assert rc == 0
    assert stdout == "".join(group_line(label, g, w) for label, g, w in zip(LABELS, cohort["groups"], cohort["want"]))
    assert len(cohort["groups"][0]) > 64
    for label, g in zip(LABELS, cohort["groups"]):
        assert read(out + "." + label) == ref_supersample(cohort["lines"], set(g)), label


@pytest.mark.parametrize("mode", [[], ["-e"], ["--unhashed"]])
def test_search_supersamples_equals_search_of_the_pooled_file(cohort, mode):
    flags = ["--junction-file", cohort["index"], "-d", "-r", "10"] + mode
    rc, got, _ = run_cli(["search", "-x", cohort["base"], "--supersamples", cohort["gpath"]] + flags)
    assert rc == 0
    rc, want, _ = run_cli(["search", "-x", cohort["base"], "--intropolis", cohort["pooled_file"]] + flags)
    assert rc == 0
    got_blocks, want_blocks = blocks(got), dict(blocks(want))
    assert [label for label, _ in got_blocks] == [int(x) for x in LABELS] and sorted(want_blocks) == [int(x) for x in LABELS]
    for label, body in got_blocks:
        assert body == want_blocks[label], (mode, label)
        assert body.count("\n") >= 1
    assert len(set(body for _, body in got_blocks)) == 3


def test_a_sum_past_int32_is_a_value_error_in_search_and_a_correct_file(tmp_path, embedded):
    lines = list(embedded["generic"])
    t = lines[16].rstrip("\n").split("\t")                      # line 16 is in every sample
    samples = [int(x) for x in t[6].split(",")]
    assert len(samples) == 10
    lines[16] = "\t".join(t[:7] + [",".join([str(BIG)] * 3 + t[7].split(",")[3:])]) + "\n"
    src, base = str(tmp_path / "big.gz"), str(tmp_path / "idx")
    _write_gz(src, lines)
    assert run_cli(["index", "--intropolis", src, "-x", base, "--features", "128", "--n-trees", "5", "-s", "10", "-t", "4",
                    "--junction-store"])[0] == 0
    gpath, out = str(tmp_path / "groups.tsv"), str(tmp_path / "pooled")
    with open(gpath, "w") as fh:
        fh.write("small\t%d\nbig\t%s\n" % (samples[0], ",".join(map(str, samples[:3]))))
    for mode in ([], ["-e"], ["--unhashed"]):
        with pytest.raises(ValueError, match=r"group big.*line 16"):
            run_cli(["search", "-x", base, "--supersamples", gpath, "--junction-file", src] + mode)
    rc, stdout, _ = run_cli(["supersample", "-x", base, "--groups", gpath, "--junction-file", src, "-o", out])
    assert rc == 0 and "# group big\tsamples 3\t" in stdout
    assert read(out + ".big") == ref_supersample(lines, samples[:3]) and read(out + ".small") == ref_supersample(lines, samples[:1])
    assert read(out + ".big").splitlines()[16].split("\t")[3] == str(3 * BIG)
