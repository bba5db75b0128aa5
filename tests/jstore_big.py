"""What the many-tile and the wide-build junction-store tests share (test_gpu_jstore_many_tiles.py,
test_gpu_jstore_build_wide.py) and what test_jstore_big_cpu.py checks without a GPU: very sparse stores of more than 64
tiles of 4096 lines with planted structure, the restatements' answers as the arrays the library returns, and the files and
the expected store of a build over more samples than the count kernel's LDS bitmap holds.  numpy only; no library call
but JunctionStore.from_arrays, which keeps a store on the host."""
import gzip

import numpy as np

from test_junctions_cpu import ref_retain

# ---- stores of many tiles ----------------------------------------------------------------------------------------------------
TILE = 4096                                 # JT_LINES: the lines of a tile of the walk
ROUND = 64                                  # tiles the tile scan takes at a time, and members a pool round takes
SIZES = [262144, 262145, 528391]            # 64 tiles: one full round; 65: a second round of one lane; 130: a third, ragged
# Pooled groups of 64 and 65 distinct members, both sides of a round, need more than 65 samples: 72 sparse ones of 200
# entries (14400 entries over up to 130 tiles: a handful of lines per sample and tile).
N_SPARSE, FIRST_ID, PER_SAMPLE = 72, 1000, 200
EMPTY, BIG = 1020, 2**31 - 1                # the sample that holds no line; the coverage three samples give BIG_LINE
BIG_IN, BIG_LINE = (1002, 1003, 1004), 262143                  # the last line of the first round's last tile
EMPTY_TILES = [(20, 27), (90, 99)]          # runs of tiles nobody holds: inside the first round, inside the second
N_DEEP, DEEP_FIRST_ID, DEEP_ENTRIES = 42, 5000, 50000          # the rows of the thinning test: 42 x 25 chunks of 2048 entries


def n_tiles(n_lines):
    return (n_lines + TILE - 1) // TILE


def planted_lines(n_lines):
    """The lines every seventh sample holds: both sides of the first tile edge and of the first round's edge, and the last."""
    return sorted(set(j for j in (0, 4095, 4096, 262143, 262144, n_lines - 1) if j < n_lines))


def free_lines(n_lines):
    """The lines outside EMPTY_TILES, ascending."""
    tile = np.arange(n_lines) // TILE
    free = np.ones(n_lines, bool)
    for first, last in EMPTY_TILES:
        free[(tile >= first) & (tile <= last)] = False
    return np.nonzero(free)[0]


def make_rows(n_lines, deep=False):
    """{sample: (lines ascending, coverages)} int64: N_SPARSE samples, ids from FIRST_ID, of PER_SAMPLE lines drawn over
    the whole range outside EMPTY_TILES; coverages 1 + geometric, a share of them on the recovery grids' thresholds.  Every
    seventh sample also holds planted_lines; EMPTY holds nothing; BIG_IN hold BIG_LINE at 2^31 - 1 each; FIRST_ID holds line
    0 at -7.  deep: N_DEEP more samples, ids from DEEP_FIRST_ID, of DEEP_ENTRIES lines and coverages 1 to 3."""
    rng = np.random.Generator(np.random.PCG64(20270 + n_lines))
    free, rows = free_lines(n_lines), {}
    for i in range(N_SPARSE):
        s = FIRST_ID + i
        line = rng.choice(free, PER_SAMPLE, replace=False)
        if i % 7 == 0:
            line = np.union1d(line, planted_lines(n_lines))
        if s in BIG_IN:
            line = np.union1d(line, [BIG_LINE])
        line = np.sort(line).astype(np.int64)
        if s == EMPTY:
            line = line[:0]
        cov = rng.geometric(0.2, len(line)).astype(np.int64)
        on_grid = rng.random(len(line)) < 0.2
        cov[on_grid] = rng.choice([2, 3, 5, 10, 20, 50, 1000], int(on_grid.sum()))
        if s in BIG_IN:
            cov[line == BIG_LINE] = BIG
        rows[s] = (line, cov)
    rows[FIRST_ID][1][0] = -7
    if deep:
        for s in range(DEEP_FIRST_ID, DEEP_FIRST_ID + N_DEEP):
            line = np.sort(rng.choice(free, DEEP_ENTRIES, replace=False)).astype(np.int64)
            rows[s] = (line, rng.integers(1, 4, len(line)).astype(np.int64))
    return rows


def sparse_ids():
    return list(range(FIRST_ID, FIRST_ID + N_SPARSE))


def deep_ids():
    return list(range(DEEP_FIRST_ID, DEEP_FIRST_ID + N_DEEP))


def make_lists(n_lines):
    """Result lists for the filter and recovery: 64 results with four ids at two ranks and EMPTY among them, 1 result, an
    empty list between two non-empty ones, the every-seventh samples (which share planted_lines), and 20 results without
    1005, the sample the recovery tests take as that list's truth."""
    rng = np.random.Generator(np.random.PCG64(31 + n_lines))
    ext = np.array(sparse_ids())
    first = rng.permutation(ext[ext != EMPTY])[:59].tolist() + [EMPTY]
    return [first + first[:4], [1003], [], ext[::7].tolist(), rng.permutation(ext[ext != 1005])[:20].tolist()]


def make_groups(n_lines):
    """Groups for the pool: 1, 64, 65 and all sparse samples -- both sides of a round of members -- and an empty group
    between them, which pins the place of the group behind it."""
    rng = np.random.Generator(np.random.PCG64(47 + n_lines))
    ext = np.array(sparse_ids())
    return [[1002], rng.permutation(ext)[:ROUND].tolist(), [], rng.permutation(ext)[:ROUND + 1].tolist(), rng.permutation(ext).tolist()]


def make_case(n_lines, deep=False):
    """The rows, their store (on the host until its first GPU call), and the lists and groups."""
    from morna_amd.junctions import JunctionStore
    rows = make_rows(n_lines, deep)
    ext = np.array(list(rows), np.int64)
    ptr = np.zeros(len(ext) + 1, np.int64)
    ptr[1:] = np.cumsum([len(rows[s][0]) for s in ext.tolist()])
    store = JunctionStore.from_arrays(ext, ptr, np.concatenate([rows[s][0] for s in ext.tolist()]),
                                      np.concatenate([rows[s][1] for s in ext.tolist()]), n_lines)
    return dict(store=store, rows=rows, n_lines=n_lines, ext=ext, lists=make_lists(n_lines), groups=make_groups(n_lines),
                cov_at={s: dict(zip(rows[s][0].tolist(), rows[s][1].tolist())) for s in sparse_ids()})


def retained_arrays(case, lst, f, c):
    """ref_retain's answer for one list as the four arrays of a Retained: lines int32 ascending, found_in words uint64,
    cov_ptr int64 from 0, coverages int32 in rank order."""
    rows, cov_at = case["rows"], case["cov_at"]
    retained, found_in = ref_retain([rows[s][0].tolist() for s in lst], [rows[s][1].tolist() for s in lst], f, c)
    lines = sorted(retained)
    masks = np.array([sum(1 << r for r in found_in[j]) for j in lines], np.uint64)
    cov_ptr = np.zeros(len(lines) + 1, np.int64)
    cov_ptr[1:] = np.cumsum([len(found_in[j]) for j in lines])
    cov = np.array([cov_at[lst[r]][j] for j in lines for r in found_in[j]], np.int32)
    return np.array(lines, np.int32), masks, cov_ptr, cov


def check_planted(case):
    """The structure make_rows promises, read from the rows and from ref_retain's answer: never from the GPU's."""
    rows, n, lists = case["rows"], case["n_lines"], case["lists"]
    tiles = n_tiles(n)
    assert tiles == {262144: 64, 262145: 65, 528391: 130}[n] and (n - 1) % TILE == {262144: 4095, 262145: 0, 528391: 6}[n]
    assert len(rows[EMPTY][0]) == 0 and rows[FIRST_ID][0][0] == 0 and rows[FIRST_ID][1][0] == -7
    for s in sparse_ids()[::7]:
        assert set(planted_lines(n)) <= set(rows[s][0].tolist())
    assert {0, 4095, 4096, 262143, n - 1} <= set(planted_lines(n)) and (262144 in planted_lines(n)) == (n > 262144)
    for s in BIG_IN:
        assert case["cov_at"][s][BIG_LINE] == BIG
    assert [len(lst) for lst in lists] == [64, 1, 0, 11, 20] and EMPTY in lists[0] and len(set(lists[0])) == 60
    assert [len(g) for g in case["groups"]] == [1, 64, 0, 65, N_SPARSE]
    # everything the 64-result list holds, by tile: runs nobody holds inside the rounds, and rounds of different totals
    lines, _, _, _ = retained_arrays(case, lists[0], 0.0, 10**6)
    per_tile = np.bincount(lines // TILE, minlength=tiles)
    held_by_anyone = np.bincount(np.concatenate([rows[s][0] for s in rows]) // TILE, minlength=tiles)
    for first, last in EMPTY_TILES:
        if last < tiles:
            assert (held_by_anyone[first:last + 1] == 0).all() and per_tile[first - 1] > 0 and per_tile[last + 1] > 0
    assert (held_by_anyone[:20] > 0).all() and held_by_anyone[tiles - 1] > 0
    rounds = [int(per_tile[r:r + ROUND].sum()) for r in range(0, tiles, ROUND)]
    assert rounds[0] > 0 and (len(rounds) == 1 or (rounds[1] > 0 and rounds[0] != sum(rounds[1:]) and rounds[0] != rounds[1]))
    return rounds


# ---- a build over more samples than the count kernel's bitmap holds ---------------------------------------------------------
WIDE_J, ALL_LINE, EDGE_LINE = 40, 20, 37    # 40 lines in blocks of 16: the line of all samples in the second, the edge line in the third
WIDE_SIZES = [262144, 262145]               # the last sample the LDS bitmap holds, and the first it does not


def first_seen(samples):
    """(ext_ids in first-seen order, the internal id of every entry) of the concatenated sample lists of a file's lines."""
    flat = np.concatenate(samples) if len(samples) else np.zeros(0, np.int64)
    uniq, first = np.unique(flat, return_index=True)
    order = np.argsort(first, kind="stable")
    rank = np.empty(len(uniq), np.int64)
    rank[order] = np.arange(len(uniq))
    return uniq[order].astype(np.int64), rank[np.searchsorted(uniq, flat)]


def wide_lines(S):
    """(samples, covs): per line of a file of WIDE_J lines over the sample ids 0 .. S - 1, the ids it lists, in the order it
    lists them, and their coverages.  ALL_LINE lists all S in a shuffled order (512 strides of the count kernel's threads);
    EDGE_LINE lists the samples of INTERNAL id S - 1, S - 32, S - 33 and 0 -- the last and first bits of the edge words of
    a bitmap of 8192 words when S is 262144 -- at coverages 2^31 - 1, 0, -5 and -2^31; the others are sparse and shuffled.
    (A line without entries cannot be written as text: the parser reads at least one sample per line.)"""
    rng = np.random.Generator(np.random.PCG64(7 + S))
    samples, covs = [], []
    for j in range(WIDE_J):
        ids = rng.permutation(S) if j == ALL_LINE else rng.choice(S, int(rng.integers(3, 40)), replace=False)
        samples.append(ids.astype(np.int64))
        covs.append(rng.integers(0, 10, len(ids)).astype(np.int64) if j == ALL_LINE else rng.geometric(0.1, len(ids)).astype(np.int64))
    ext, _ = first_seen(samples[:ALL_LINE + 1])                # every sample has its internal id by the end of ALL_LINE
    assert len(ext) == S
    samples[EDGE_LINE] = ext[[S - 1, S - 32, S - 33, 0]]
    covs[EDGE_LINE] = np.array([BIG, 0, -5, -2**31], np.int64)
    return samples, covs


def write_lines(path, samples, covs):
    """The lines as a gzip intropolis file: eight tab-separated columns, distinct keys."""
    with gzip.open(path, "wt", compresslevel=1) as fh:
        for j, (ids, c) in enumerate(zip(samples, covs)):
            fh.write("chr1\t%d\t%d\t+\tGT\tAG\t%s\t%s\n" % (1000 + 10 * j, 1500 + 10 * j, ",".join(map(str, ids.tolist())),
                                                            ",".join(map(str, c.tolist()))))


def expected_store(samples, covs):
    """The store of a file as a stable sort of its entries by sample: (ext_ids in first-seen order, ptr from bincount, lines
    ascending inside a sample, coverages carried along)."""
    ext, internal = first_seen(samples)
    line = np.repeat(np.arange(len(samples)), [len(ids) for ids in samples])
    order = np.argsort(internal, kind="stable")
    ptr = np.zeros(len(ext) + 1, np.int64)
    ptr[1:] = np.cumsum(np.bincount(internal, minlength=len(ext)))
    cov = np.concatenate(covs) if len(covs) else np.zeros(0, np.int64)
    return ext, ptr, line[order].astype(np.int32), cov[order].astype(np.int32)


def store_file_bytes(ext, ptr, line, cov, n_lines):
    """The bytes JunctionStore.save writes for these arrays (csrc/jstore.hip: magic, three counts, the four arrays)."""
    return b"MORNAJS1" + np.array([len(ext), len(line), n_lines], "<i8").tobytes() + np.asarray(ext, "<i8").tobytes() \
        + np.asarray(ptr, "<i8").tobytes() + np.asarray(line, "<i4").tobytes() + np.asarray(cov, "<i4").tobytes()


def with_repeat(ids, c, x, times=1):
    """A line's lists with sample x appended until it stands `times` more often than once."""
    extra = times + (0 if x in ids.tolist() else 1)
    return np.concatenate([ids, np.full(extra, x, np.int64)]), np.concatenate([c, np.full(extra, 9, np.int64)])
