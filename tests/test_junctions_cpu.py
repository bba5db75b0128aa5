"""`morna junctions` without a GPU: the parser, the splice-file writer, min_count and the store file.

The yardstick of the junction logic is `ref_junctions` below: a line-for-line restatement of the reference's retention
step and output loop (commanderson/morna morna.py:1539-1629) that works on the text lines with dicts and sets as the
reference does.  The reference itself cannot run (Python 2, annoy / mmh3 / BitVector absent) and holds no recorded
`junctions` output; the GPU tests (test_gpu_junctions.py) compare whole splice files with this restatement.
"""
import gzip
import os
from collections import defaultdict
from math import ceil

import numpy as np
import pytest

from conftest import GOLDEN


# ---- the restatement ---------------------------------------------------------------------------------------------------
def sample_lists(lines):
    """What the reference's per-sample tables hold (morna.py:221-341, read back at 1516-1532): for every sample id of ANY
    line, its line numbers (0-based, ascending) and its coverages there, as the strings of the text."""
    juncs, covrs = defaultdict(list), defaultdict(list)
    for i, line in enumerate(lines):
        tokens = line.strip().split("\t")
        for sample, coverage in zip(tokens[6].split(","), tokens[7].split(",")):
            juncs[int(sample)].append(i)
            covrs[int(sample)].append(coverage)
    return juncs, covrs


def ref_retain(result_juncs, result_covrs, frequency_filter, coverage_filter):
    """morna.py:1539-1569: result_juncs[r] / result_covrs[r] are result r's line numbers and coverages (strings, as the
    reference splits them out of its tables).  Returns (retain_junctions, found_in_map)."""
    retain_junctions = set()
    frequency_counts = defaultdict(int)
    found_in_map = defaultdict(list)
    min_count = int(ceil(frequency_filter * len(result_juncs)))
    for i, junction_list in enumerate(result_juncs):
        for index in junction_list:
            frequency_counts[index] += 1
            found_in_map[index].append(i)
    if result_juncs:        # (the reference repeats this identical pass once per result, morna.py:1556)
        for index in frequency_counts:
            if frequency_counts[index] >= min_count:
                retain_junctions.add(index)
    for i, coverages_list in enumerate(result_covrs):
        for j, coverage in enumerate(coverages_list):
            if int(coverage) >= coverage_filter:
                retain_junctions.add(result_juncs[i][j])
    return retain_junctions, found_in_map


def ref_junctions(lines, result_sample_ids, f, c, tables=None):
    """morna.py:1539-1629 for one result list (external sample ids in rank order).  Returns dict(text: the splice file,
    count: len(retain_junctions), lines / found_in / covs: what the output loop used, for the writer's tests)."""
    juncs, covrs = tables if tables is not None else sample_lists(lines)
    result_juncs = [juncs[s] for s in result_sample_ids]
    result_covrs = [covrs[s] for s in result_sample_ids]
    retain_junctions, found_in_map = ref_retain(result_juncs, result_covrs, f, c)
    ordered_junctions = sorted(retain_junctions)
    out, out_found, out_covs = [], [], []
    for i in ordered_junctions:          # (the reference walks the file and pops the next index, morna.py:1588-1635)
        line = lines[i]
        retain_sample_ids = []
        for result_index in found_in_map[i]:
            retain_sample_ids.append(result_sample_ids[result_index])
        tokens = line.strip().split("\t")
        tokens[1] = str(int(tokens[1]) - 2)
        old_samples = [int(x) for x in tokens[6].split(",")]
        old_covs = [int(x) for x in tokens[7].split(",")]
        new_samples = []
        new_covs = []
        for sample_id in retain_sample_ids:
            if sample_id in old_samples:
                new_samples.append(sample_id)
                new_covs.append(old_covs[old_samples.index(sample_id)])
        tokens[6] = ",".join([str(_) for _ in new_samples])
        tokens[7] = ",".join([str(_) for _ in new_covs])
        out.append("\t".join(tokens) + "\t" + str(found_in_map[i]) + "\n")
        out_found.append(list(found_in_map[i]))
        out_covs.append(new_covs)
    return dict(text="".join(out), count=len(retain_junctions), lines=ordered_junctions, found_in=out_found, covs=out_covs)


def retained_from_ref(ref):
    """The restatement's answer as the arrays the library returns (junctions.Retained)."""
    from morna_amd.junctions import Retained
    masks = np.array([sum(1 << r for r in ranks) for ranks in ref["found_in"]], np.uint64)
    cov_ptr = np.zeros(len(ref["lines"]) + 1, np.int64)
    cov_ptr[1:] = np.cumsum([len(c) for c in ref["covs"]])
    cov = np.array([c for row in ref["covs"] for c in row], np.int32)
    return Retained(np.array(ref["lines"], np.int32), masks, cov_ptr, cov)


def tiny_lines():
    with open(os.path.join(GOLDEN, "tiny_intropolis.tsv")) as fh:
        return fh.readlines()


def store_arrays(lines):
    """The store of `lines` as from_arrays takes it: samples in first-seen order."""
    juncs, covrs = sample_lists(lines)
    ext = list(juncs)
    ptr = np.zeros(len(ext) + 1, np.int64)
    ptr[1:] = np.cumsum([len(juncs[s]) for s in ext])
    line = np.array([j for s in ext for j in juncs[s]], np.int32)
    cov = np.array([int(c) for s in ext for c in covrs[s]], np.int32)
    return np.array(ext, np.int64), ptr, line, cov, len(lines)


# ---- parser --------------------------------------------------------------------------------------------------------------
def test_junctions_parser_flags_and_defaults():
    from morna_amd import cli
    p = cli.build_parser()
    a = p.parse_args(["junctions", "-x", "idx", "--junction-file", "j.gz", "-sf", "out.txt"])
    assert a.subparser_name == "junctions"
    assert a.pass1_sam == "pass1.sam" and a.junction_filter == ".05,5" and a.index is None     # morna.py:1025-1053
    assert a.junction_file == "j.gz" and a.splicefile == "out.txt"
    s = p.parse_args(["search", "-x", "idx"])
    for name, value in vars(s).items():                  # all of search's parameters, with search's defaults
        if name != "subparser_name":
            assert getattr(a, name) == value, name
    a = p.parse_args(["junctions", "-x", "idx", "--junction-file", "j.gz", "--splicefile", "o", "-p1", "first.sam", "-i", "hg38",
                      "--junction-filter", ".5,3", "-q", "7", "-e", "--device", "1", "--query-ids", "1,2", "-r", "5"])
    assert (a.pass1_sam, a.index, a.junction_filter, a.query_id, a.exact, a.device, a.results) == \
        ("first.sam", "hg38", ".5,3", 7, True, "1", 5)
    a = p.parse_args(["index", "--intropolis", "f.gz", "--junction-store"])
    assert a.junction_store is True
    assert p.parse_args(["index", "--intropolis", "f.gz"]).junction_store is False


@pytest.mark.parametrize("argv", [
    ["junctions", "-x", "idx", "-sf", "out.txt"],                                              # no --junction-file
    ["junctions", "-x", "idx", "--junction-file", "j.gz"],                                     # no --splicefile
    ["junctions", "-x", "idx", "--junction-file", "j.gz", "-sf", "o", "--junction-filter", "5"],
    ["junctions", "-x", "idx", "--junction-file", "j.gz", "-sf", "o", "--junction-filter", "a,5"],
    ["junctions", "-x", "idx", "--junction-file", "j.gz", "-sf", "o", "--junction-filter", ".05,1.5"],
    ["junctions", "-x", "idx", "--junction-file", "j.gz", "-sf", "o", "--junction-filter", ".05,5,1"],
    ["junctions", "-x", "idx", "--junction-file", "j.gz", "-sf", "o", "-c", "10"],
    ["junctions", "-x", "idx", "--junction-file", "j.gz", "-sf", "o", "--intropolis", "q.gz", "-q", "3"],
])
def test_junctions_parser_errors(argv, capsys):
    from morna_amd import cli
    with pytest.raises(SystemExit) as e:
        cli.main(argv)
    assert e.value.code == 2
    capsys.readouterr()


def test_junction_filter_parts():
    from morna_amd.junctions import parse_junction_filter
    assert parse_junction_filter(".05,5") == (0.05, 5)
    assert parse_junction_filter("1.0,1000") == (1.0, 1000)
    assert parse_junction_filter("0,1000") == (0.0, 1000)


# ---- min_count -----------------------------------------------------------------------------------------------------------
def test_min_count_edge_values(embedded):
    from morna_amd.junctions import min_count
    for m in (1, 5, 20, 64):
        assert min_count(0, m) == 0 and min_count(0.0, m) == 0
        assert min_count(1.0, m) == m
    assert min_count(0.05, 20) == 1
    assert min_count(0.3, 7) == 3                       # 0.3 * 7 = 2.1 -> 3
    assert min_count(.05, 5) == 1 and min_count(.5, 5) == 3
    # what those values mean, through the restatement: 0 keeps every junction at least one result holds, 1.0 only
    # those all m results hold (the coverage part switched off by a filter no coverage reaches)
    lines = embedded["generic"]
    juncs, _ = sample_lists(lines)
    results = [8, 3, 5, 1, 10, 2, 7]
    present = sorted(set(j for s in results for j in juncs[s]))
    assert ref_junctions(lines, results, 0, 10**9)["lines"] == present
    in_all = [j for j in present if all(j in juncs[s] for s in results)]
    assert ref_junctions(lines, results, 1.0, 10**9)["lines"] == in_all
    in_three = [j for j in present if sum(j in juncs[s] for s in results) >= 3]
    assert ref_junctions(lines, results, 0.3, 10**9)["lines"] == in_three and in_all != in_three != present


# ---- the writer ----------------------------------------------------------------------------------------------------------
def _write(path, lines, gz):
    if gz:
        with gzip.open(path, "wt") as fh:
            fh.write("".join(lines))
    else:
        with open(path, "w") as fh:
            fh.write("".join(lines))


@pytest.mark.parametrize("gz", [True, False])
def test_writer_equals_restatement_on_generic(tmp_path, embedded, gz):
    from morna_amd.junctions import write_splice_files
    lines = embedded["generic"]
    src = str(tmp_path / "j")
    _write(src, lines, gz)
    tables = sample_lists(lines)
    jobs, want = [], []
    for n, (results, f, c) in enumerate([([1, 2, 3, 4, 5], .05, 5), ([10, 9, 8], .5, 3), ([5, 1, 7, 3, 9, 2], 1.0, 1000),
                                         ([4, 6, 8, 10], 0, 1000), ([2], 1.0, 10**9), ([], .05, 5)]):
        ref = ref_junctions(lines, results, f, c, tables)
        jobs.append((str(tmp_path / ("out%d" % n)), retained_from_ref(ref), results))
        want.append(ref["text"])
    assert any(w == "" for w in want) and any(w.count("\n") > 3 for w in want)
    write_splice_files(src, jobs)                      # one pass over the file for all of them
    for (path, _, _), text in zip(jobs, want):
        with open(path) as fh:
            assert fh.read() == text


def test_writer_equals_restatement_on_tiny(tmp_path):
    from morna_amd.junctions import write_splice_files
    lines = tiny_lines()
    src = str(tmp_path / "tiny.gz")
    _write(src, lines, True)
    tables = sample_lists(lines)
    samples = sorted(tables[0])
    results = samples[:3] + samples[1000:1010] + samples[-7:]
    ref = ref_junctions(lines, results, .05, 5, tables)
    assert ref["count"] == 3
    out = str(tmp_path / "splices")
    write_splice_files(src, [(out, retained_from_ref(ref), results)])
    with open(out) as fh:
        got = fh.read()
    assert got == ref["text"]
    first = got.split("\n")[0].split("\t")
    assert len(first) == 9 and int(first[1]) == int(lines[0].split("\t")[1]) - 2 and first[8].startswith("[")


def test_writer_rejects_a_file_that_was_not_indexed(tmp_path, embedded):
    from morna_amd.junctions import write_splice_files
    lines = embedded["generic"]
    ref = ref_junctions(lines, [1, 2, 3, 4, 5], 0, 1000)
    other = list(lines)
    t = other[16].rstrip("\n").split("\t")               # the line all ten samples share: another coverage for sample 2
    covs = t[7].split(",")
    covs[t[6].split(",").index("2")] = str(int(covs[t[6].split(",").index("2")]) + 1)
    other[16] = "\t".join(t[:7] + [",".join(covs)]) + "\n"
    src = str(tmp_path / "other.gz")
    _write(src, other, True)
    with pytest.raises(ValueError, match="line 16 "):
        write_splice_files(src, [(str(tmp_path / "o1"), retained_from_ref(ref), [1, 2, 3, 4, 5])])
    short = str(tmp_path / "short.gz")
    _write(short, lines[:10], True)
    with pytest.raises(ValueError, match="ends before line"):
        write_splice_files(short, [(str(tmp_path / "o2"), retained_from_ref(ref), [1, 2, 3, 4, 5])])


# ---- the store file (no device: load and from_arrays keep the store on the host until the first retain) -------------------
def test_store_round_trip(tmp_path, embedded):
    from morna_amd.junctions import JunctionStore
    for name, lines in (("generic", embedded["generic"]), ("tiny", tiny_lines())):
        ext, ptr, line, cov, n_lines = store_arrays(lines)
        a = JunctionStore.from_arrays(ext, ptr, line, cov, n_lines)
        assert (a.n_samples, a.nnz, a.n_lines) == (len(ext), len(line), n_lines)
        path = str(tmp_path / (name + ".junc.mor"))
        a.save(path)
        b = JunctionStore.load(path)
        assert (b.n_samples, b.nnz, b.n_lines) == (a.n_samples, a.nnz, a.n_lines)
        assert b.sample_ids().tolist() == ext.tolist()
        juncs, covrs = sample_lists(lines)
        for s in ext.tolist()[:50] + ext.tolist()[-5:]:
            got_line, got_cov = b.sample(s)
            assert got_line.tolist() == juncs[s] and got_cov.tolist() == [int(c) for c in covrs[s]]
        again = str(tmp_path / (name + ".again"))
        b.save(again)
        with open(path, "rb") as f1, open(again, "rb") as f2:
            assert f1.read() == f2.read()
        with pytest.raises(IndexError, match="424242"):
            b.sample(424242)


def test_store_rejects_inconsistent_arrays(embedded):
    from morna_amd.junctions import JunctionStore
    ext, ptr, line, cov, n_lines = store_arrays(embedded["generic"])
    JunctionStore.from_arrays(ext, ptr, line, cov, n_lines)
    bad = ptr.copy()
    bad[3], bad[4] = ptr[4], ptr[3]
    with pytest.raises(ValueError):
        JunctionStore.from_arrays(ext, bad, line, cov, n_lines)                 # ptr not monotone
    s = int(np.argmax(np.diff(ptr) >= 2))
    bad = line.copy()
    bad[ptr[s]], bad[ptr[s] + 1] = line[ptr[s] + 1], line[ptr[s]]
    with pytest.raises(ValueError):
        JunctionStore.from_arrays(ext, ptr, bad, cov, n_lines)                  # lines descend inside a sample
    bad[ptr[s]] = bad[ptr[s] + 1]
    with pytest.raises(ValueError):
        JunctionStore.from_arrays(ext, ptr, bad, cov, n_lines)                  # a line twice
    with pytest.raises(ValueError):
        JunctionStore.from_arrays(ext, ptr, line, cov, int(line.max()))         # a line at n_lines
    bad = ext.copy()
    bad[1] = bad[0]
    with pytest.raises(ValueError):
        JunctionStore.from_arrays(bad, ptr, line, cov, n_lines)                 # sample ids not distinct


def test_store_load_rejects_damaged_files(tmp_path, embedded):
    from morna_amd.junctions import JunctionStore
    ext, ptr, line, cov, n_lines = store_arrays(embedded["generic"])
    path = str(tmp_path / "g.junc.mor")
    JunctionStore.from_arrays(ext, ptr, line, cov, n_lines).save(path)
    with open(path, "rb") as fh:
        blob = fh.read()
    assert len(blob) == 8 + 24 + 8 * len(ext) + 8 * (len(ext) + 1) + 8 * len(line)
    head = 32

    def load(data):
        p = str(tmp_path / "damaged.junc.mor")
        with open(p, "wb") as fh:
            fh.write(data)
        return JunctionStore.load(p)
    load(blob)
    with pytest.raises(IOError):
        JunctionStore.load(str(tmp_path / "missing.junc.mor"))
    for data in (blob[:-1], blob[:40], b"", blob + b"\0", b"MORNAJS0" + blob[8:]):
        with pytest.raises(IOError):
            load(data)
    as_i64 = np.frombuffer(blob[head:head + 8 * (2 * len(ext) + 1)], np.int64).copy()
    tail = blob[head + 8 * (2 * len(ext) + 1):]
    dup = as_i64.copy()
    dup[1] = dup[0]                                                             # ext_ids not distinct
    with pytest.raises(IOError):
        load(blob[:head] + dup.tobytes() + tail)
    unsorted = as_i64.copy()
    unsorted[len(ext) + 2] = as_i64[len(ext) + 3] + 1                           # ptr not monotone
    with pytest.raises(IOError):
        load(blob[:head] + unsorted.tobytes() + tail)
    lines32 = np.frombuffer(tail[:4 * len(line)], np.int32).copy()
    lines32[int(np.argmax(line))] = n_lines                                     # a line at n_lines
    with pytest.raises(IOError):
        load(blob[:head] + as_i64.tobytes() + lines32.tobytes() + tail[4 * len(line):])
    s = int(np.argmax(np.diff(ptr) >= 2))
    lines32 = np.frombuffer(tail[:4 * len(line)], np.int32).copy()
    lines32[ptr[s] + 1] = lines32[ptr[s]]                                       # lines not ascending inside a sample
    with pytest.raises(IOError):
        load(blob[:head] + as_i64.tobytes() + lines32.tobytes() + tail[4 * len(line):])


def test_retain_rejects_more_than_64_results(embedded):
    """The limit is checked before any GPU work: 65 results per list fail with a message that names 64."""
    from morna_amd.junctions import JunctionStore
    ext, ptr, line, cov, n_lines = store_arrays(embedded["generic"])
    store = JunctionStore.from_arrays(ext, ptr, line, cov, n_lines)
    with pytest.raises(ValueError, match="64"):
        store.retain([[1] * 65], .05, 5)


def test_stale_store_is_removed(tmp_path):
    from morna_amd.junctions import STORE_SUFFIX, remove_stale_store
    base = str(tmp_path / "idx")
    remove_stale_store(base)                            # nothing there: nothing happens
    with open(base + STORE_SUFFIX, "wb") as fh:
        fh.write(b"x")
    remove_stale_store(base)
    assert not os.path.exists(base + STORE_SUFFIX)
