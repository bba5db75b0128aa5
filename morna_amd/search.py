"""Host side of `morna search`: the counterpart of MornaSearch.

Mirrors commanderson/morna morna.py:522-787: same constructor (loads the index
file set written by MornaIndex.save), same `update_query` / `finalize_query` /
`search_nn` / `exact_search_nn` / `search_member_n` signatures and return
shapes, same errors.  Query construction (a dict of summed coverages, then one
hash + idf per distinct junction) stays in Python exactly as in the reference;
the searches run in libmorna_hip.so.

`meta_db=True` appends the keywords of `<basename>.meta.mor` to the results
(morna.py:666-676; metadb.py).

Batch form (no counterpart in the reference, which answers one query sample per
process): `queries_from_intropolis` featurises every sample of an intropolis file
against the index's vocabulary -- a native pre-pass, then the rows on the GPU --
and `search_nn_batch` / `exact_search_nn_batch` answer all of them in one call,
each exactly as `update_query` over that sample's lines, `finalize_query` and
`search_nn` / `exact_search_nn` would.
"""
import os
import pickle
import sys
from collections import defaultdict
from math import log

import numpy as np

from . import _lib
from .annoy import LABEL_SUMS_STATS, MIXTURE_STATS, AnnoyIndex
from .metadb import lookup_meta


def results_output(results, out=None):
    """Human-readable result lines (morna.py:116-127)."""
    out = out or sys.stdout
    for i in range(len(results[0])):
        out.write(str(i + 1) + ".")
        for lst in results:
            out.write("\t" + str(lst[i]))
        out.write("\n")


INT32_MAX = 2**31 - 1

SHARDS_REFUSAL = ("restricted search (--within, --without, --leave-out-groups) is not available on an index of row shards "
                  "(.shards.mor, one process per shard, --device a,b): run it on an index built without --shards")


def restriction_arrays(internal_id_map, n_items, within=None, without=None, groups=None):
    """The host side of MornaSearch.restriction: EXTERNAL sample ids -> (allow, item_group, n_groups) over the n_items
    internal ids.  allow: booleans [n_items] -- `within` (None: every item) less `without` -- or None when neither is
    given; item_group: int32 [n_items], the position of an item's group in `groups` ([(label, [ids])]) or -1, or None when
    groups is None.  ValueError naming the id for an id the index lacks, and for an id in two groups."""
    def internal(sample_id, what):
        if sample_id not in internal_id_map:
            raise ValueError("%s names sample id %s, which is not in the index" % (what, sample_id))
        i = internal_id_map[sample_id]
        if not 0 <= i < n_items:
            raise ValueError("%s names sample id %s, whose internal id %d is outside the index's %d items"
                             % (what, sample_id, i, n_items))
        return i
    allow = None
    if within is not None or without is not None:
        allow = np.ones(n_items, bool)
        if within is not None:
            allow[:] = False
            for sample_id in within:
                allow[internal(sample_id, "within")] = True
        for sample_id in (without or ()):
            allow[internal(sample_id, "without")] = False
    item_group, n_groups = None, 0
    if groups is not None:
        groups = list(groups)
        n_groups = len(groups)
        item_group = np.full(n_items, -1, np.int32)
        for g, (label, ids) in enumerate(groups):
            for sample_id in ids:
                i = internal(sample_id, "group %s" % label)
                if item_group[i] >= 0 and item_group[i] != g:
                    raise ValueError("sample id %s is in two groups, %s and %s" % (sample_id, groups[item_group[i]][0], label))
                item_group[i] = g
    return allow, item_group, n_groups


def restricted_search_k(n_trees, k, n_items, n_allowed):
    """The default search_k of a search under an allow-list: annoy's n_trees * k scaled by ceil(n / n_allowed), so that the
    traversal collects about as many ALLOWED candidates as the unrestricted default collects candidates; at most 2^31 - 1.
    (A deliberate departure from annoy's default; an explicit search_k is taken as given.)"""
    scale = -(-int(n_items) // max(int(n_allowed), 1))
    return min(int(n_trees) * int(k) * scale, INT32_MAX)


RADIUS_SHARDS_REFUSAL = ("radius search (--max-distance, pairs) is not available on an index of row shards (.shards.mor, one "
                         "process per shard, --device a,b): run it on an index built without --shards")


def parse_max_distance(text):
    """--max-distance: a finite distance >= 0 (the angular distance lies in [0, 2]; 2 and more returns every sample)."""
    try:
        d = float(text)
    except (TypeError, ValueError):
        raise ValueError("--max-distance takes a distance, a finite number >= 0 such as 0.15 (got %r)" % (text,))
    if not (d >= 0.0) or d == float("inf"):
        raise ValueError("--max-distance takes a distance, a finite number >= 0 such as 0.15 (got %r)" % (text,))
    return d


def sort_pairs(pairs):
    """(idA, idB, distance) triples in the order `morna pairs` prints them: NaN pairs first, then by (distance, idA, idB)."""
    return sorted(pairs, key=lambda p: (0, 0.0, p[0], p[1]) if p[2] != p[2] else (1, p[2], p[0], p[1]))


def pair_clusters(pairs):
    """The connected components of the graph whose edges are `pairs` ((idA, idB, ...) tuples): a list of id lists, every
    list ascending, the largest component first (equal sizes: by their smallest id).  Union-find on the host."""
    parent = {}

    def find(x):
        root = x
        while parent[root] != root:
            root = parent[root]
        while parent[x] != root:
            parent[x], x = root, parent[x]
        return root
    for p in pairs:
        a, b = p[0], p[1]
        parent.setdefault(a, a)
        parent.setdefault(b, b)
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    members = defaultdict(list)
    for x in parent:
        members[find(x)].append(x)
    return sorted((sorted(m) for m in members.values()), key=lambda m: (-len(m), m[0]))


def format_distance(d):
    """A distance as `search -d` prints it (str of the float); nan for a NaN."""
    return "nan" if d != d else str(float(d))


def format_pair_line(id_a, id_b, d, meta=None):
    """One line of `morna pairs`: idA<TAB>idB<TAB>distance, and with meta = (keywords of A, keywords of B) both appended."""
    line = "%s\t%s\t%s" % (id_a, id_b, format_distance(d))
    if meta is not None:
        line += "\t%s\t%s" % (meta[0], meta[1])
    return line + "\n"


def format_pairs_summary(n_samples, pairs, clusters):
    """The summary line of `morna pairs`."""
    return "# samples %d\tpairs %d\tsamples in any pair %d\tlargest cluster %d\n" % (
        n_samples, len(pairs), sum(len(c) for c in clusters), len(clusters[0]) if clusters else 0)


def format_cluster_line(cluster):
    return "# cluster %d\t%s\n" % (len(cluster), ",".join(str(i) for i in cluster))


TREES_SHARDS_REFUSAL = ("a search over the first trees of the forest (n_trees=, --use-trees, recall) is not available on an index "
                        "of row shards (.shards.mor, one process per shard, --device a,b): run it on an index built without "
                        "--shards")
SWEEP_MAX_LIST = 64
RECALL_MAX_K = 256


def parse_int_list(text, what, all_value=None):
    """"10,20,all" -> [10, 20, all_value]: a comma-separated list of positive integers, strictly ascending, 1 to 64 entries;
    the literal `all` stands for all_value (the index's tree count) where one is given.  ValueError says what is wrong."""
    out = []
    for token in str(text).split(","):
        token = token.strip()
        if token == "all" and all_value is not None:
            out.append(int(all_value))
            continue
        try:
            value = int(token)
        except ValueError:
            raise ValueError("%s: %r is not an integer" % (what, token))
        if value < 1:
            raise ValueError("%s: %d is not positive" % (what, value))
        out.append(value)
    if len(out) > SWEEP_MAX_LIST:
        raise ValueError("%s: %d entries, at most %d are taken" % (what, len(out), SWEEP_MAX_LIST))
    for a, b in zip(out, out[1:]):
        if b <= a:
            raise ValueError("%s: %d follows %d, the entries must ascend strictly" % (what, b, a))
    return out


def recall_rows(trees, search_ks, hits, exact_count, ncand, ndots, q):
    """The lines of one query's block of `morna recall`: per cell (trees, search_k, hits, exact results, recall, candidates,
    hyperplane dots); recall is hits / exact results (0.0 when the exact search found nothing), None -- with hits -1 --
    when the exact search failed for the query."""
    rows = []
    for i, t in enumerate(trees):
        for j, s in enumerate(search_ks):
            h, e = int(hits[i][j][q]), int(exact_count[q])
            recall = None if h < 0 else (float(h) / e if e > 0 else 0.0)
            rows.append((int(t), int(s), h, e, recall, int(ncand[i][j][q]), int(ndots[i][j][q])))
    return rows


def recall_summary(trees, search_ks, hits, exact_count, ncand, ndots):
    """(rows, failed): per cell (trees, search_k, mean recall, minimum recall, queries with recall 1, mean
    candidates, mean hyperplane dots) over the queries whose exact search succeeded (hits >= 0); `failed` is the number left
    out.  With no query counted the means are None."""
    hits, ncand, ndots = np.asarray(hits), np.asarray(ncand), np.asarray(ndots)
    exact_count = np.asarray(exact_count)
    nq = len(exact_count)
    rows = []
    ok = [q for q in range(nq) if exact_count[q] >= 0]
    for i, t in enumerate(trees):
        for j, s in enumerate(search_ks):
            rec = [r[4] for r in (recall_rows(trees[i:i + 1], search_ks[j:j + 1], hits[i:i + 1, j:j + 1], exact_count,
                                              ncand[i:i + 1, j:j + 1], ndots[i:i + 1, j:j + 1], q)[0] for q in ok)]
            if not ok:
                rows.append((int(t), int(s), None, None, 0, None, None))
                continue
            rows.append((int(t), int(s), sum(rec) / len(ok), min(rec), sum(1 for r in rec if r == 1.0),
                         float(sum(int(ncand[i][j][q]) for q in ok)) / len(ok), float(sum(int(ndots[i][j][q]) for q in ok)) / len(ok)))
    return rows, nq - len(ok)


def format_recall_rows(rows):
    """One tab-separated line per row of recall_rows / recall_summary: floats with six digits, None as "nan"."""
    def cell(v):
        if v is None:
            return "nan"
        return "%.6f" % v if isinstance(v, float) else str(v)
    return "".join("\t".join(cell(v) for v in row) + "\n" for row in rows)


HASHING_SHARDS_REFUSAL = ("hashing is not available on an index of row shards (.shards.mor, one process per shard, --device a,b): "
                          "run it on an index built without --shards")
HASHING_MAX_DIMS = 16
HASHING_MAX_FEATURES = 32768
HASHING_SEARCH_K = 100          # morna's default: search --search-k


def parse_features_list(text, index_dim=None):
    """--features "500,1000,index" of `morna hashing` -> [500, 1000, index_dim]: parse_int_list's ascending positive
    integers, `index` the index's own width; at most 16 entries, each 1 to 32768.  ValueError says what is wrong."""
    tokens = [t.strip() for t in str(text).split(",")]
    if index_dim is None and "index" in tokens:
        raise ValueError("--features: 'index' needs an index to stand for")
    dims = parse_int_list(",".join(str(int(index_dim)) if t == "index" else t for t in tokens), "--features")
    if len(dims) > HASHING_MAX_DIMS:
        raise ValueError("--features: %d entries, at most %d are taken" % (len(dims), HASHING_MAX_DIMS))
    for d in dims:
        if d > HASHING_MAX_FEATURES:
            raise ValueError("--features: %d is above %d, the widest row an index takes" % (d, HASHING_MAX_FEATURES))
    return dims


def drop_query(ids, dists, me, r):
    """A result list without the query `me` and without the -1 of a short list, cut to r: the `others` of
    scripts/recall_vs_unhashed.py, with the distances kept beside the ids."""
    kept = [(int(i), float(d)) for i, d in zip(ids, dists) if int(i) != int(me) and int(i) >= 0][:int(r)]
    return [i for i, _ in kept], [d for _, d in kept]


def _hashing_cells(truth, found):
    """(hits, recall, dist_err) of one found list against the truth, both (ids, distances)."""
    t_ids, t_d = truth
    f_ids, f_d = found
    at = dict(zip(f_ids, f_d))
    shared = [(t_d[j], at[i]) for j, i in enumerate(t_ids) if i in at]
    hits = len(shared)
    recall = float(hits) / len(t_ids) if len(t_ids) else None
    dist_err = sum(abs(h - u) for u, h in shared) / hits if hits else None
    return hits, recall, dist_err


def hashing_rows(dims, truth, exact, approx=None):
    """The lines of one query's block of `morna hashing`.  truth: (ids, distances) of the unhashed search with the query
    dropped; exact[i] / approx[i]: the same of the exact / the forest search in the dims[i]-wide hashed space (approx None
    without --n-trees).  Per D: (features, truth, hits, recall, dist_err[, hits_approx, recall_approx]); recall is None when
    the truth is empty, dist_err -- the mean of abs(hashed distance - unhashed distance) over the shared ids -- None when
    there are none."""
    rows = []
    for i, d in enumerate(dims):
        hits, recall, dist_err = _hashing_cells(truth, exact[i])
        row = (int(d), len(truth[0]), hits, recall, dist_err)
        if approx is not None:
            a_hits, a_recall, _ = _hashing_cells(truth, approx[i])
            row += (a_hits, a_recall)
        rows.append(row)
    return rows


def norm_ratio_stats(norm2, pp):
    """(mean, population variance) of sqrt(norm2) / sqrt(pp) over the items with pp != 0: how well the hashed rows keep the
    norms of the unhashed ones (the reference's test_norm_estimator.py with the vector's norm divided out).  (None, None)
    when no item has a norm."""
    norm2, pp = np.asarray(norm2, np.float64), np.asarray(pp, np.float64)
    keep = pp != 0.0
    if not keep.any():
        return None, None
    ratio = np.sqrt(norm2[keep]) / np.sqrt(pp[keep])
    mean = float(ratio.sum() / len(ratio))
    return mean, float(((ratio - mean) ** 2).sum() / len(ratio))


def hashing_summary(tables, norm_stats):
    """The block over all queries from the queries' own (hashing_rows): per D the truths and hits summed, recall their
    quotient, dist_err the mean of the queries' dist_err (those that have one), then norm_stats[i] = (norm_ratio_mean,
    norm_ratio_var) of that D."""
    tables = list(tables)
    out = []
    for i, cell in enumerate(zip(*tables)):
        truth, hits = sum(r[1] for r in cell), sum(r[2] for r in cell)
        errs = [r[4] for r in cell if r[4] is not None]
        row = (cell[0][0], truth, hits, float(hits) / truth if truth else None, sum(errs) / len(errs) if errs else None)
        if len(cell[0]) > 5:
            a_hits = sum(r[5] for r in cell)
            row += (a_hits, float(a_hits) / truth if truth else None)
        out.append(row + tuple(norm_stats[i]))
    return out


def format_hashing_rows(rows):
    """One tab-separated line per row of hashing_rows / hashing_summary: floats with six digits, None as "-"."""
    def cell(v):
        if v is None:
            return "-"
        return "%.6f" % v if isinstance(v, float) else str(v)
    return "".join("\t".join(cell(v) for v in row) + "\n" for row in rows)


LABELS_SHARDS_REFUSAL = ("labels is not available on an index of row shards (.shards.mor, one process per shard, --device a,b): "
                         "run it on an index built without --shards")
LABELS_MAX = 4096               # MORNA_LABELS_MAX: a workgroup keeps every label's sum and count on chip
LABELS_FIXED_ONE = 4294967296.0  # the sums are fixed point with 32 fractional bits
LABELS_CALL_CELLS = 1 << 22     # (query, label) cells of one library call: 48 MiB of outputs


def labels_max_refusal(n_labels):
    return ("--labels names %d labels, at most %d are taken: the GPU keeps one sum and one count per label on chip while it "
            "reads a query's distances" % (n_labels, LABELS_MAX))


def label_means(sums_q, counts_q):
    """m[g] = sums / 2^32 / counts of one query, None where the query counts no sample of the label."""
    return [int(s) / LABELS_FIXED_ONE / int(c) if int(c) > 0 else None for s, c in zip(sums_q, counts_q)]


def label_query(sums_q, counts_q, own=None):
    """What one query's sums say: means (label_means), predicted (the label of the smallest mean, ties to the lowest label
    index, None when no label is counted) and, for a query whose own label `own` (None or negative: none) is counted beside
    at least one other: a (the mean to its own label), other and b (the nearest other label and the mean to it), silhouette
    (b - a) / max(a, b) (0.0 when both are 0) and agree (predicted == own).  Without them the silhouette is None."""
    means = label_means(sums_q, counts_q)
    counted = [g for g, m in enumerate(means) if m is not None]
    out = dict(means=means, predicted=min(counted, key=lambda g: (means[g], g)) if counted else None,
               own=None if own is None or own < 0 else int(own), a=None, other=None, b=None, silhouette=None, agree=None)
    own = out["own"]
    others = [g for g in counted if g != own]
    if own is None or means[own] is None or not others:
        return out
    other = min(others, key=lambda g: (means[g], g))
    a, b = means[own], means[other]
    out.update(a=a, other=other, b=b, silhouette=(b - a) / max(a, b) if max(a, b) > 0 else 0.0, agree=out["predicted"] == own)
    return out


def label_rows(names, sums_q, counts_q, own=None, top=3):
    """The lines of one query's block of `morna labels`: the `top` nearest labels as ("<rank>.", label, count, mean distance)
    and, where label_query defines a silhouette, ("silhouette", own label, own count, a, nearest other label, b, silhouette,
    agree 0 | 1)."""
    info = label_query(sums_q, counts_q, own)
    means = info["means"]
    order = sorted((g for g, m in enumerate(means) if m is not None), key=lambda g: (means[g], g))
    rows = [("%d." % (rank + 1), names[g], int(counts_q[g]), means[g]) for rank, g in enumerate(order[:max(int(top), 0)])]
    if info["silhouette"] is not None:
        rows.append(("silhouette", names[info["own"]], int(counts_q[info["own"]]), info["a"], names[info["other"]], info["b"],
                     info["silhouette"], 1 if info["agree"] else 0))
    return rows


def label_summary(names, sums, counts, own=None):
    """(rows, without) over all queries.  own: the own label of every query (by-item queries; negative: none) -- then one row
    per label that has queries with a silhouette, in file order, (label, queries, mean a, mean b, mean silhouette, queries
    that agree, their share), an ("all", ...) row over those queries when there are any, and `without`, the number of queries
    without a silhouette.  own None (queries from outside the index): (label, queries predicted to it) per label, and
    `without` the queries that count no labelled sample at all."""
    if own is None:
        predicted = [label_query(sums[q], counts[q])["predicted"] for q in range(len(sums))]
        return [(names[g], sum(1 for p in predicted if p == g)) for g in range(len(names))], sum(1 for p in predicted if p is None)
    infos = [label_query(sums[q], counts[q], own[q]) for q in range(len(sums))]
    defined = [i for i in infos if i["silhouette"] is not None]

    def row(label, group):
        n = len(group)
        agree = sum(1 for i in group if i["agree"])
        return (label, n, sum(i["a"] for i in group) / n, sum(i["b"] for i in group) / n, sum(i["silhouette"] for i in group) / n,
                agree, float(agree) / n)
    rows = []
    for g in range(len(names)):
        group = [i for i in defined if i["own"] == g]
        if group:
            rows.append(row(names[g], group))
    if defined:
        rows.append(row("all", defined))
    return rows, len(infos) - len(defined)


def label_map(n_labels, sums, counts, own):
    """M[A][B]: the mean of m[q][B] over the queries of own label A that count a sample of B; None where no query does."""
    total = [[0.0] * n_labels for _ in range(n_labels)]
    seen = [[0] * n_labels for _ in range(n_labels)]
    for q in range(len(sums)):
        a = int(own[q])
        if a < 0:
            continue
        for b, m in enumerate(label_means(sums[q], counts[q])):
            if m is not None:
                total[a][b] += m
                seen[a][b] += 1
    return [[total[a][b] / seen[a][b] if seen[a][b] else None for b in range(n_labels)] for a in range(n_labels)]


def format_label_rows(rows):
    """One tab-separated line per row of label_rows / label_summary / the label map: floats with six digits, None as "nan"."""
    return format_recall_rows(rows)


# ---- morna mixture ----------------------------------------------------------------------------------
MIXTURE_SHARDS_REFUSAL = ("mixture is not available on an index of row shards (.shards.mor, one process per shard, --device a,b): "
                          "run it on an index built without --shards")
MIXTURE_LABELS_MAX = 128        # MORNA_MIXTURE_LABELS_MAX: the normalised Gram matrix of the labels stays on chip
MIXTURE_CALL_CELLS = 1 << 22    # (query, label) cells of one library call


def mixture_max_refusal(n_labels):
    return ("--labels names %d labels, mixture takes 1 to %d: the GPU keeps the labels' Gram matrix on chip while it fits a "
            "query" % (n_labels, MIXTURE_LABELS_MAX))


def mixture_shares(weights_q):
    """share[g] = weight / the sum of the weights (added in file order); all 0.0 when no weight is positive."""
    total = 0.0
    for w in weights_q:
        total += float(w)
    return [float(w) / total if total > 0.0 else 0.0 for w in weights_q]


def mixture_query(weights_q, min_share=0.1):
    """What one query's weights say: shares (mixture_shares), order (the labels of positive weight, the largest first, ties in
    file order), top (order[0] or None) and mixed (a second label holds a share of at least min_share)."""
    shares = mixture_shares(weights_q)
    order = sorted((g for g, w in enumerate(weights_q) if float(w) > 0.0), key=lambda g: (-float(weights_q[g]), g))
    return dict(shares=shares, order=order, top=order[0] if order else None,
                mixed=len(order) >= 2 and shares[order[1]] >= min_share)


def format_mixture_header(query_id, own_name, info_q):
    """The first line of a query's block of `morna mixture`; info_q: rr, kkt, sweeps, status."""
    rr = float(info_q[0])
    return "# query %s\tlabel %s\tresidual %.6f\tsweeps %d\tconverged %d\n" % (
        query_id, "-" if own_name is None else own_name, max(rr, 0.0) ** 0.5, int(info_q[2]), 1 if info_q[3] == 1 else 0)


def mixture_rows(names, weights_q, top=3, min_share=0.1):
    """The lines of one query's block behind its header: the `top` labels by weight as ("<rank>.", label, weight, share), then
    ("mixed", 1 | 0)."""
    info = mixture_query(weights_q, min_share)
    rows = [("%d." % (rank + 1), names[g], float(weights_q[g]), info["shares"][g])
            for rank, g in enumerate(info["order"][:max(int(top), 0)])]
    rows.append(("mixed", 1 if info["mixed"] else 0))
    return rows


def mixture_summary(names, weights, info, own=None, min_share=0.1):
    """(rows, without) over all queries.  own: the own label of every query (by-item queries; negative: none) -- then one row
    per label that has queries, in file order, (label, queries, mean share of the own label, queries whose own label is on top,
    mixed queries, queries that did not converge), an ("all", ...) row over those queries when there are any, and `without`,
    the queries without an own label.  own None (queries from outside the index): (label, queries whose top label it is) per
    label, then ("mixed", their number); `without`: the queries with no positive weight."""
    per = [mixture_query(weights[q], min_share) for q in range(len(weights))]
    if own is None:
        rows = [(names[g], sum(1 for p in per if p["top"] == g)) for g in range(len(names))]
        rows.append(("mixed", sum(1 for p in per if p["mixed"])))
        return rows, sum(1 for p in per if p["top"] is None)

    def row(label, group):
        n = len(group)
        return (label, n, sum(per[q]["shares"][int(own[q])] for q in group) / n,
                sum(1 for q in group if per[q]["top"] == int(own[q])), sum(1 for q in group if per[q]["mixed"]),
                sum(1 for q in group if info[q][3] != 1))
    rows, labelled = [], [q for q in range(len(per)) if int(own[q]) >= 0]
    for g in range(len(names)):
        group = [q for q in labelled if int(own[q]) == g]
        if group:
            rows.append(row(names[g], group))
    if labelled:
        rows.append(row("all", labelled))
    return rows, len(per) - len(labelled)


def mixture_matrix(n_labels, weights, own):
    """M[A][B]: the mean share of label B over the queries whose own label is A; None where A has no query."""
    total = [[0.0] * n_labels for _ in range(n_labels)]
    seen = [0] * n_labels
    for q in range(len(weights)):
        a = int(own[q])
        if a < 0:
            continue
        seen[a] += 1
        for b, s in enumerate(mixture_shares(weights[q])):
            total[a][b] += s
    return [[total[a][b] / seen[a] if seen[a] else None for b in range(n_labels)] for a in range(n_labels)]


# ---- morna cluster ----------------------------------------------------------------------------------
CLUSTER_SHARDS_REFUSAL = ("cluster is not available on an index of row shards (.shards.mor, one process per shard, --device a,b): "
                          "run it on an index built without --shards")
CLUSTER_MAX_VALUES = 1 << 29    # k * samples: the scan values of all centroids share one batch of 2 GiB


def cluster_max_refusal(k, n_eligible):
    return ("cluster takes 1 to %d clusters, and no more than the %d samples it partitions (got %d): every cluster is a label "
            "that `labels --labels` can read" % (LABELS_MAX, n_eligible, k))


def cluster_seed_items(eligible, k, seed):
    """The first centroids of `morna cluster --seed`: random.Random(seed).sample of the eligible INTERNAL ids in ascending
    order, k of them."""
    import random
    eligible = sorted(int(i) for i in eligible)
    if not 1 <= k <= len(eligible):
        raise ValueError(cluster_max_refusal(k, len(eligible)))
    return random.Random(seed).sample(eligible, k)


def cluster_label(j):
    return "c%04d" % j


def cluster_table(assign, dist, k):
    """Per cluster of an assignment (assign[i] in [-1, k), dist[i] the member's distance): (size, mean member distance,
    centre), the mean summed on the host in ascending id and None for an empty cluster, the centre the member (an INTERNAL
    id) with the smallest distance, the lowest id on ties, a NaN behind every number, None for an empty cluster."""
    size, total, centre, best = [0] * k, [0.0] * k, [None] * k, [None] * k
    for i, (j, d) in enumerate(zip(assign.tolist(), dist.tolist())):
        if j < 0:
            continue
        size[j] += 1
        total[j] += d
        if centre[j] is None or d < best[j] or (best[j] != best[j] and d == d):
            centre[j], best[j] = i, d
    return [(size[j], total[j] / size[j] if size[j] else None, centre[j]) for j in range(k)]


def format_clusters_header(k, iterations, converged, n_samples, mean):
    """The first line of `morna cluster`."""
    return "# clusters %d\titerations %d\tconverged %s\tsamples %d\tmean distance %s\n" % (
        k, iterations, "yes" if converged else "no", n_samples, format_distance(mean))


def format_clusters_row(label, size, mean, centre, meta=None):
    """One line per cluster: label, size, mean member distance, centre sample ('-' for both in an empty cluster), and with
    meta (a string) that sample's keywords."""
    line = "%s\t%d\t%s\t%s" % (label, size, "-" if mean is None else format_distance(mean), "-" if centre is None else centre)
    if meta is not None:
        line += "\t%s" % meta
    return line + "\n"


def format_clusters_sample(sample_id, label, d):
    return "%s\t%s\t%s\n" % (sample_id, label, format_distance(d))


def write_groups_file(path, groups):
    """[(label, [ids])] as the groups file junctions.parse_groups_file reads back unchanged."""
    with open(path, "w") as fh:
        for label, ids in groups:
            fh.write("%s\t%s\n" % (label, ",".join(str(i) for i in ids)))


PCA_SHARDS_REFUSAL = ("pca is not available on an index of row shards (.shards.mor, one process per shard, --device a,b): "
                      "run it on an index built without --shards")
PCA_MAX_COMPONENTS = 32         # MORNA_PCA_MAX_COMPONENTS
PCA_MAX_BLOCK = 64              # MORNA_PCA_MAX_BLOCK: components and extra columns together
PCA_CALL_VALUES = 1 << 24       # row elements of one projection call


def pca_width_refusal(p, extra):
    return ("pca takes 1 to %d components and, with --extra, a block of at most %d columns (got -p %d --extra %d)"
            % (PCA_MAX_COMPONENTS, PCA_MAX_BLOCK, p, extra))


def format_pca_header(p, iterations, converged, n_samples, total_variance):
    """The first line of `morna pca`."""
    return "# pca %d\titerations %d\tconverged %s\tsamples %d\ttotal variance %s\n" % (
        p, iterations, "yes" if converged else "no", n_samples, format_distance(total_variance))


def pca_shares(values, total_variance):
    """[(variance, share of the total variance, cumulative share)] per component, the cumulative share summed in order;
    NaN shares where the total variance is not positive."""
    rows, running = [], 0.0
    for v in values:
        share = float(v) / total_variance if total_variance > 0.0 else float("nan")
        running += share
        rows.append((float(v), share, running))
    return rows


def format_pca_components(values, total_variance):
    """One "# pc<j>" line per component: variance, share, cumulative share."""
    return "".join("# pc%d\t%s\t%s\t%s\n" % (j + 1, format_distance(v), format_distance(share), format_distance(cum))
                   for j, (v, share, cum) in enumerate(pca_shares(values, total_variance)))


def format_pca_row(name, coords, label=None, meta=None):
    """id<TAB>[label<TAB>]c1<TAB>..<TAB>cp and, with meta (a string), the keywords."""
    fields = [str(name)] + ([str(label)] if label is not None else []) + [format_distance(c) for c in coords]
    if meta is not None:
        fields.append(meta)
    return "\t".join(fields) + "\n"


def pca_label_means(names, item_label, coords):
    """[(label, members with coordinates, mean coordinates or None)] in the order of `names`: the mean of the members'
    coordinates summed on the host in ascending internal id, a member with NaN coordinates left out."""
    p = coords.shape[1]
    out = []
    for l, name in enumerate(names):
        total, count = [0.0] * p, 0
        for i in np.nonzero(item_label == l)[0].tolist():
            row = coords[i].tolist()
            if row[0] != row[0]:
                continue
            count += 1
            for j in range(p):
                total[j] += row[j]
        out.append((name, count, [t / count for t in total] if count else None))
    return out


def format_pca_label_means(means):
    """The block of per-label mean coordinates: "# label means", then label<TAB>members<TAB>c1..cp ('-' without a member)."""
    lines = ["# label means\n"]
    for name, count, mean in means:
        lines.append("%s\t%d\t%s\n" % (name, count, "-" if mean is None else "\t".join(format_distance(c) for c in mean)))
    return "".join(lines)


def save_pca_axes(path, pca, dim):
    """The axes of a SearchPCA as one .npz: mean, axes, values, info (iterations, converged, fitted, total variance) and dim.
    Written to exactly `path`."""
    info = np.array([pca.iterations, 1.0 if pca.converged else 0.0, pca.fitted, pca.total_variance], np.float64)
    with open(path, "wb") as fh:
        np.savez(fh, mean=np.asarray(pca.mean, np.float64), axes=np.asarray(pca.axes, np.float64),
                 values=np.asarray(pca.values, np.float64), info=info, dim=np.array(dim, np.int64))


def load_pca_axes(path, dim):
    """The SearchPCA (without samples) that save_pca_axes wrote; ValueError for a file that lacks an array, whose arrays do
    not fit each other, or that was made for an index of another dimension."""
    with np.load(path, allow_pickle=False) as z:
        missing = [k for k in ("mean", "axes", "values", "info", "dim") if k not in z.files]
        if missing:
            raise ValueError("%s is no file of --save-axes: it lacks %s" % (path, ", ".join(missing)))
        mean, axes, values, info, file_dim = (np.asarray(z[k]) for k in ("mean", "axes", "values", "info", "dim"))
    if int(file_dim) != dim:
        raise ValueError("%s holds axes of dimension %d, the index has %d" % (path, int(file_dim), dim))
    if axes.ndim != 2 or axes.shape[1] != dim or mean.shape != (dim,) or values.shape != (axes.shape[0],) or info.shape != (4,):
        raise ValueError("%s is no file of --save-axes: its arrays do not fit each other" % path)
    return SearchPCA(axes.astype(np.float64), mean.astype(np.float64), values.astype(np.float64), int(info[0]), bool(info[1]),
                     int(info[2]), float(info[3]), None)


def accumulate_stats(total, last, maxima=()):
    """The statistics of one more call (a *_stats dict) into those of a scan made of several: every key summed, the keys of
    `maxima` the largest seen."""
    for key, value in last.items():
        total[key] = max(total[key], value) if key in maxima else total[key] + value


def vectors_or_items(queries):
    """The queries of a label scan that are no QueryBatch, under the keyword AnnoyIndex takes them by: ("Q", fp64 vectors
    [nq, dim]) for a 2-d array, else ("items", int32 INTERNAL ids [nq])."""
    if isinstance(queries, np.ndarray) and queries.ndim == 2:
        return "Q", np.ascontiguousarray(queries, dtype=np.float64)
    return "items", np.array(list(queries), np.int32).reshape(-1)


def chunked_call(call, nq, step, outs):
    """call(q0, q1) for the queries [q0, q1) of every chunk of `step`, in order; what it returns, one array per entry of
    `outs`, is stored to their rows [q0, q1)."""
    for q0 in range(0, nq, step):
        q1 = min(q0 + step, nq)
        for out, part in zip(outs, call(q0, q1)):
            out[q0:q1] = part


class SearchClusters(object):
    """MornaSearch.cluster_samples: groups [(label, [EXTERNAL ids])] with the members in ascending internal id; per cluster
    sizes, means (mean member distance, None when empty) and centres (EXTERNAL id of the member nearest its centroid, None
    when empty); samples [(EXTERNAL id, cluster, distance)] in ascending internal id; iterations, converged, n_samples, the
    mean distance over all samples, and stats (AnnoyIndex.kmeans_stats)."""

    def __init__(self, groups, sizes, means, centres, samples, iterations, converged, stats):
        self.groups, self.sizes, self.means, self.centres, self.samples = groups, sizes, means, centres, samples
        self.iterations, self.converged, self.stats = iterations, converged, stats
        self.n_samples = len(samples)
        total = 0.0
        for _, _, d in samples:
            total += d
        self.mean = total / self.n_samples if self.n_samples else float("nan")

    def header(self):
        return format_clusters_header(len(self.groups), self.iterations, self.converged, self.n_samples, self.mean)

    def rows(self, meta=None):
        """The per-cluster lines; meta: {EXTERNAL id: keywords} for the centre samples, or None."""
        return "".join(format_clusters_row(label, size, mean, centre, None if meta is None else meta.get(centre, "-"))
                       for (label, _), size, mean, centre in zip(self.groups, self.sizes, self.means, self.centres))

    def sample_lines(self):
        return "".join(format_clusters_sample(sample_id, self.groups[j][0], d) for sample_id, j, d in self.samples)


class SearchPCA(object):
    """MornaSearch.principal_axes: axes (float64 [p, dim]), mean ([dim]), values ([p], the variances), iterations, converged,
    fitted (the rows that took part), total_variance and stats (AnnoyIndex.pca_stats; None for axes read from a file);
    after MornaSearch.pca_samples also samples (EXTERNAL ids in ascending internal id) and coords (float64 [n, p])."""

    def __init__(self, axes, mean, values, iterations, converged, fitted, total_variance, stats):
        self.axes, self.mean, self.values = axes, mean, values
        self.iterations, self.converged, self.fitted, self.total_variance, self.stats = iterations, converged, fitted, total_variance, stats
        self.samples, self.coords = None, None

    def header(self):
        return format_pca_header(len(self.values), self.iterations, self.converged, self.fitted, self.total_variance)

    def components(self):
        return format_pca_components(self.values, self.total_variance)

    def sample_lines(self, labels=None, meta=None):
        """A line per indexed sample; labels: {EXTERNAL id: label} ('-' for a sample without one), meta: {EXTERNAL id: keywords}."""
        return "".join(format_pca_row(sample_id, row, None if labels is None else labels.get(sample_id, "-"),
                                      None if meta is None else meta.get(sample_id, "-"))
                       for sample_id, row in zip(self.samples, self.coords.tolist()))


class SearchLabels(object):
    """MornaSearch.label_separation: names (the labels in file order), item_label (int32 [n], -1: none), sums (uint64) and
    counts (int32) [nq, L] as AnnoyIndex.label_sums returns them, own (the own label of every by-item query, None for queries
    from outside the index) and stats (AnnoyIndex.label_sums_stats summed over the calls)."""

    def __init__(self, names, item_label, sums, counts, own, stats):
        self.names, self.item_label, self.sums, self.counts, self.own, self.stats = names, item_label, sums, counts, own, stats

    def rows(self, q, top=3):
        return label_rows(self.names, self.sums[q], self.counts[q], None if self.own is None else self.own[q], top)

    def own_name(self, q):
        return None if self.own is None or self.own[q] < 0 else self.names[int(self.own[q])]

    def summary(self):
        return label_summary(self.names, self.sums, self.counts, self.own)

    def map(self):
        return label_map(len(self.names), self.sums, self.counts, self.own)


class SearchMixture(object):
    """MornaSearch.label_mixture: names (the labels in file order), item_label (int32 [n], -1: none), weights (float64 [nq, L]),
    info (float64 [nq, 4]: squared residual, KKT residual, sweeps, status), active (bool [nq, L]), own (the own label of every
    by-item query, None for queries from outside the index) and stats (AnnoyIndex.mixture_stats summed over the calls)."""

    def __init__(self, names, item_label, weights, info, active, own, stats):
        self.names, self.item_label, self.weights, self.info, self.active = names, item_label, weights, info, active
        self.own, self.stats = own, stats

    def own_name(self, q):
        return None if self.own is None or self.own[q] < 0 else self.names[int(self.own[q])]

    def header(self, q, query_id):
        return format_mixture_header(query_id, self.own_name(q), self.info[q])

    def rows(self, q, top=3, min_share=0.1):
        return mixture_rows(self.names, self.weights[q], top, min_share)

    def summary(self, min_share=0.1):
        return mixture_summary(self.names, self.weights, self.info, self.own, min_share)

    def matrix(self):
        return mixture_matrix(len(self.names), self.weights, self.own)


class SearchHashing(object):
    """MornaSearch.hashing_sweep: dims, tables[q] (hashing_rows of query q), norm_stats[i] of dims[i], and kernel_ms[i], the
    time of the rows' kernel at dims[i]."""

    def __init__(self, dims, tables, norm_stats, kernel_ms):
        self.dims, self.tables, self.norm_stats, self.kernel_ms = list(dims), tables, norm_stats, kernel_ms

    def rows(self, q):
        return self.tables[q]

    def summary(self):
        return hashing_summary(self.tables, self.norm_stats)


class SearchRecall(object):
    """MornaSearch.search_recall: trees, search_ks, and per cell hits / ncand / ndots [n_t, n_s, nq], exact_count [nq]."""

    def __init__(self, trees, search_ks, out):
        self.trees, self.search_ks = list(trees), list(search_ks)
        self.hits, self.exact_count, self.ncand, self.ndots = out["hits"], out["exact_count"], out["ncand"], out["ndots"]

    def rows(self, q):
        return recall_rows(self.trees, self.search_ks, self.hits, self.exact_count, self.ncand, self.ndots, q)

    def summary(self):
        return recall_summary(self.trees, self.search_ks, self.hits, self.exact_count, self.ncand, self.ndots)


class SearchRestriction(object):
    """MornaSearch.restriction: allow (booleans [n] or None), item_group (int32 [n] or None), the counts, and `handle`,
    the annoy.Restriction on the index's device."""

    def __init__(self, owner, handle, allow, item_group, n_groups):
        self.owner, self.handle, self.allow, self.item_group, self.n_groups = owner, handle, allow, item_group, n_groups
        self.n_items, self.n_allowed = handle.n_items, handle.n_allowed

    def summary(self):
        return "restriction: %d of %d samples allowed, %d leave-out groups" % (self.n_allowed, self.n_items, self.n_groups)

    def own_groups(self, internal_ids):
        """g_q of by-member queries: every query carries its own item's label (None without groups)."""
        if self.item_group is None:
            return None
        return self.item_group[np.asarray(internal_ids, np.int64)]


class QueryBatch(object):
    """The query samples of an intropolis file featurised against an index (MornaSearch.queries_from_intropolis):
    ext_ids[q] is the sample id of query q (first appearance in the file), n the number of queries.  The rows live on
    the index's handle (a later queries_from_intropolis replaces them); rows64 / rows32 are host copies for an index of
    row shards, which searches from host memory."""

    def __init__(self, owner, generation, ext_ids, rows64=None, rows32=None):
        self.owner, self.generation = owner, generation
        self.ext_ids = [int(x) for x in ext_ids]
        self.n = len(self.ext_ids)
        self.rows64, self.rows32 = rows64, rows32


class MornaSearch(object):
    def __init__(self, basename, device=0, rank=None, world=None):
        """rank / world: one process per shard of an index built with --shards (shards.DistShards); None: this process
        holds the whole index (or all of its shards, shards.LocalShards)."""
        self.basename = basename
        self._device = int(device[0] if isinstance(device, (list, tuple)) else device)
        self._junction_store = None
        with open(basename + ".stats.mor") as stats_stream:
            self.sample_count = int(stats_stream.readline())
            self.index_size = int(stats_stream.readline())
            self.dim = int(stats_stream.readline())
        self.query = defaultdict(int)
        self.query_sample = [0.0 for _ in range(self.dim)]
        if world is not None and world > 1:                    # torchrun: this process serves shard `rank`
            from .shards import DistShards
            self.annoy_index = DistShards(basename, self.dim, rank, world, device=device)
        elif os.path.exists(basename + ".shards.mor"):         # written by `morna index --shards G` (index.py)
            from .shards import LocalShards
            self.annoy_index = LocalShards(basename, self.dim, device=device)
        else:
            self.annoy_index = AnnoyIndex(self.dim, metric="angular", device=device)
            self.annoy_index.load(basename + '.annoy.mor')
        with open(basename + ".freq.mor", "rb") as pickle_stream:
            self.sample_frequencies = defaultdict(int, pickle.load(pickle_stream))
        with open(basename + ".map.mor", "rb") as pickle_stream:
            self.internal_id_map = pickle.load(pickle_stream)

    def inverse_lookup(self, internal_id):
        """External sample id that owns `internal_id`, None when nobody does (contract of morna.py:552-572:
        the map is one-to-one, a second owner is a RuntimeError)."""
        owners = [sample_id for sample_id, mapped in self.internal_id_map.items() if mapped == internal_id]
        if len(owners) > 1:
            raise RuntimeError(str(internal_id) + " does not have unique mapping in self.internal_id_map.")
        return owners[0] if owners else None

    def update_query(self, junction):
        """Sum the coverage of one (chrom, start, end, coverage, ...) junction (morna.py:597-607)."""
        self.query[tuple(junction[:3])] += int(junction[3])

    def finalize_query(self):
        """query_sample from the summed coverages (arithmetic contract of morna.py:609-629).

        One term per distinct junction, in the dict's insertion order: weight = log(sample_count / df) with the
        index's FINAL document frequency of the key "chrom start end" (0 for a junction the index never saw),
        term = coverage * weight, added with the sign of the key's 32-bit hash into column hash mod dim (Python's
        floored modulo), all in fp64 -- the terms a column receives are added in that order.
        """
        hash32 = _lib.lib().morna_hash32
        dense = [0.0] * self.dim
        for parts, coverage in self.query.items():
            text = ' '.join(map(str, parts))
            df = self.sample_frequencies.get(text, 0)
            weight = log(float(self.sample_count) / df) if df else 0
            raw = text.encode("ascii")
            h = int(hash32(raw, len(raw)))          # mmh3.hash: signed
            term = coverage * weight
            dense[h % self.dim] += -term if h < 0 else term
        self.query_sample = dense

    def _with_meta(self, results, meta_db):
        """Append the metadata keywords of each result (morna.py:666-676)."""
        if not meta_db:
            return results
        sample_ids = [self.inverse_lookup(internal_id) for internal_id in results[0]]
        return results + (lookup_meta(self.basename, sample_ids),)

    def _check_trees(self, n_trees, restriction=None):
        """n_trees= of the searches: None, or a count the one-handle index searches the first trees with."""
        if n_trees is None:
            return
        if restriction is not None:
            raise ValueError("n_trees cannot be used with a restriction")
        if not isinstance(self.annoy_index, AnnoyIndex):
            raise ValueError(TREES_SHARDS_REFUSAL)

    def search_nn(self, num_neighbors, search_k, include_distances=True, meta_db=False, restriction=None, n_trees=None):
        """Approximate neighbours of query_sample (morna.py:632-678); restriction: MornaSearch.restriction; n_trees: search
        the first n_trees trees only -- the answer of an index built with --n-trees n_trees."""
        self._check_trees(n_trees, restriction)
        if n_trees is not None:
            ids, d, cnt = self.annoy_index.get_nns_by_vector_batch(np.array([self.query_sample], dtype=np.float32), num_neighbors,
                                                                   search_k, n_trees=n_trees)
            return self._batch_results(ids, d, cnt, include_distances, meta_db)[0]
        if restriction is not None:
            self._check_restriction(restriction, None)
            ids, d, cnt = self.annoy_index.get_nns_restricted(
                restriction.handle, num_neighbors, self._restricted_search_k(restriction, num_neighbors, search_k),
                Q=np.array([self.query_sample], dtype=np.float32))
            return self._batch_results(ids, d, cnt, include_distances, meta_db)[0]
        if include_distances:
            results = self.annoy_index.get_nns_by_vector([feature for feature in self.query_sample],
                                                         num_neighbors, search_k, include_distances)
        else:
            results = (self.annoy_index.get_nns_by_vector([feature for feature in self.query_sample],
                                                          num_neighbors, search_k, include_distances),)
        return self._with_meta(results, meta_db)

    def exact_search_nn(self, num_neighbors, include_distances=True, meta_db=False, restriction=None):
        """Brute-force neighbours with cosine_distance (morna.py:681-730); restriction: MornaSearch.restriction."""
        if restriction is not None:
            self._check_restriction(restriction, None)
            ids, d, cnt = self.annoy_index.exact_search_restricted(restriction.handle, num_neighbors,
                                                                   Q=np.array([self.query_sample], dtype=np.float64))
        else:
            ids, d, cnt = self.annoy_index.exact_search_batch(np.array([self.query_sample], dtype=np.float64),
                                                              num_neighbors)
        m = int(cnt[0])
        if m < 0:
            # some indexed row gives cosine_distance a negative radicand: the reference's math.sqrt raises while it
            # walks the rows (morna.py:101-114, 697-700), whatever that row's rank would have been
            raise ValueError("math domain error")
        results = ([int(x) for x in ids[0, :m]],)
        if include_distances:
            results += ([float(x) for x in d[0, :m]],)
        return self._with_meta(results, meta_db)

    # ---- many query samples at once ---------------------------------------------------------------------------
    def _vocab(self):
        """The frequency table as the arrays of the native pre-pass, made once."""
        if getattr(self, "_vocab_arrays", None) is None:
            from .index import pack_vocab
            self._vocab_arrays = pack_vocab(self.sample_frequencies)
        return self._vocab_arrays

    def _device_index(self, shards_refusal=None):
        """What every batch call asks first: RuntimeError with one process per shard (torchrun); with shards_refusal, that
        ValueError on any other index of row shards."""
        from .shards import DistShards
        if isinstance(self.annoy_index, DistShards):
            raise RuntimeError("batch search is not available with one process per shard (torchrun): "
                               "run it in one process, which loads every shard of the index")
        if shards_refusal is not None and not isinstance(self.annoy_index, AnnoyIndex):
            raise ValueError(shards_refusal)

    def _check_batch_possible(self):
        self._device_index()
        if self.sample_count <= 0:
            raise ValueError("the index's sample count must be positive (got %d)" % self.sample_count)

    def queries_from_intropolis(self, path):
        """Every sample of the (gzipped) intropolis file `path` as a query: for sample s, the vector update_query over
        the lines that list s (key "chrom start end" in the index's frequency table, coverage of s) and finalize_query
        would make -- built on the GPU.  Coordinates are compared as written (intropolis writes canonical decimals,
        what the raw stream's int() gives).  Returns a QueryBatch."""
        from .index import ParsedLines
        self._check_batch_possible()
        parsed = ParsedLines(path, sample_count=self.sample_count, sample_threshold=0)
        return self._batch_from_terms(parsed.query_terms(self._vocab(), self.sample_count))

    def _batch_from_terms(self, terms):
        """The QueryBatch of the query terms of a parse (ParsedLines.query_terms): its rows built on the GPU."""
        from .shards import LocalShards
        ext_ids = terms.arrays()["ext_ids"].tolist()
        self._batch_generation = getattr(self, "_batch_generation", 0) + 1
        if isinstance(self.annoy_index, LocalShards):
            # the rows are built on shard 0's device and searched from the host by every shard
            handle = self.annoy_index.shards[0]
            handle.build_query_rows(terms)
            rows64, rows32 = handle.get_query_rows()
            return QueryBatch(self, self._batch_generation, ext_ids, rows64, rows32)
        self.annoy_index.build_query_rows(terms)
        return QueryBatch(self, self._batch_generation, ext_ids)

    def _check_batch(self, batch):
        if batch.owner is not self or batch.generation != getattr(self, "_batch_generation", 0):
            raise ValueError("the rows of this query batch were replaced by a later queries_from_intropolis call")

    def _inverse_map(self):
        """internal id -> external sample id, made once (inverse_lookup's contract: a second owner is an error)."""
        if getattr(self, "_inverse", None) is None:
            inv = {}
            for sample_id, internal_id in self.internal_id_map.items():
                if internal_id in inv:
                    raise RuntimeError(str(internal_id) + " does not have unique mapping in self.internal_id_map.")
                inv[internal_id] = sample_id
            self._inverse = inv
        return self._inverse

    def _result_rows(self, lists, counts, include_distances, meta_db):
        """One result per (ids, distances) list, shaped as search_nn / exact_search_nn return it; where the count is negative
        (an exact query the reference raises on) a ValueError instance."""
        inv = self._inverse_map() if meta_db else None
        out = []
        for (ids, d), m in zip(lists, counts):
            if int(m) < 0:
                out.append(ValueError("math domain error"))
                continue
            results = ([int(x) for x in ids],)
            if include_distances:
                results += ([float(x) for x in d],)
            if meta_db:
                results += (lookup_meta(self.basename, [inv.get(i) for i in results[0]]),)
            out.append(results)
        return out

    def _batch_results(self, ids, d, cnt, include_distances, meta_db):
        """_result_rows for the padded arrays of the *_batch searches: row q holds cnt[q] results."""
        return self._result_rows([(ids[q, :max(int(m), 0)], d[q, :max(int(m), 0)]) for q, m in enumerate(cnt)], cnt, include_distances,
                                 meta_db)

    # ---- restricted search -------------------------------------------------------------------
    def restriction(self, within=None, without=None, groups=None):
        """A SearchRestriction for the *_batch searches' restriction=: EXTERNAL sample ids.  The searches answer only with
        the samples of `within` (None: all) that are not in `without`; groups, [(label, [ids])] as parse_groups_file returns
        it, are leave-out groups: a query that carries a group (query_groups=, or a by-member query's own) gets no member of
        it back.  ValueError for an id the index lacks, for an id in two groups, and on an index of row shards."""
        if not isinstance(self.annoy_index, AnnoyIndex):
            raise ValueError(SHARDS_REFUSAL)
        n = self.annoy_index.get_n_items()
        allow, item_group, n_groups = restriction_arrays(self.internal_id_map, n, within, without, groups)
        return SearchRestriction(self, self.annoy_index.restriction(allow, item_group), allow, item_group, n_groups)

    def _check_restriction(self, restriction, query_groups):
        if restriction is None:
            if query_groups is not None:
                raise ValueError("query_groups needs a restriction made with groups")
            return
        if not isinstance(restriction, SearchRestriction) or restriction.owner is not self:
            raise ValueError("the restriction was not made by this MornaSearch (MornaSearch.restriction)")

    def _restricted_search_k(self, restriction, num_neighbors, search_k):
        """search_k None or -1 under an allow-list: restricted_search_k; anything else as given."""
        if search_k is None or search_k == -1:
            if restriction.allow is None:
                return -1
            return restricted_search_k(self.annoy_index.get_n_trees(), num_neighbors, restriction.n_items, restriction.n_allowed)
        return search_k

    def _unhashed_population_of(self, restriction):
        """_unhashed_population narrowed to the allowed samples (the unhashed search takes its population from the host)."""
        pop = self._unhashed_population()
        if restriction is None or restriction.allow is None:
            return pop
        self._check_restriction(restriction, None)
        return pop[restriction.allow]

    def search_nn_batch(self, batch, num_neighbors, search_k, include_distances=True, meta_db=False, restriction=None,
                        query_groups=None, n_trees=None):
        """search_nn for every query of `batch`: a list of result tuples, in query order.  restriction / query_groups:
        MornaSearch.restriction and the group label every query carries (positions in its groups, negative: none);
        n_trees: as search_nn."""
        self._check_batch(batch)
        self._check_restriction(restriction, query_groups)
        self._check_trees(n_trees, restriction)
        if n_trees is not None:
            ids, d, cnt = self.annoy_index.get_nns_by_query_rows(num_neighbors, search_k, n_trees=n_trees)
            return self._batch_results(ids, d, cnt, include_distances, meta_db)
        if restriction is not None:
            ids, d, cnt = self.annoy_index.get_nns_restricted(
                restriction.handle, num_neighbors, self._restricted_search_k(restriction, num_neighbors, search_k),
                query_groups=query_groups)
            return self._batch_results(ids, d, cnt, include_distances, meta_db)
        if batch.rows32 is not None:
            ids, d, cnt = self.annoy_index.get_nns_by_vector_batch(batch.rows32, num_neighbors, search_k)
        else:
            ids, d, cnt = self.annoy_index.get_nns_by_query_rows(num_neighbors, search_k)
        return self._batch_results(ids, d, cnt, include_distances, meta_db)

    def exact_search_nn_batch(self, batch, num_neighbors, include_distances=True, meta_db=False, restriction=None,
                              query_groups=None):
        """exact_search_nn for every query of `batch`: a list of result tuples, in query order; a query the reference
        would raise on gets a ValueError instance in its slot.  restriction / query_groups: as search_nn_batch; the answer
        is then the reference's on an index of the eligible samples only."""
        self._check_batch(batch)
        self._check_restriction(restriction, query_groups)
        if restriction is not None:
            ids, d, cnt = self.annoy_index.exact_search_restricted(restriction.handle, num_neighbors, query_groups=query_groups)
            return self._batch_results(ids, d, cnt, include_distances, meta_db)
        if batch.rows64 is not None:
            ids, d, cnt = self.annoy_index.exact_search_batch(batch.rows64, num_neighbors)
        else:
            ids, d, cnt = self.annoy_index.exact_search_query_rows(num_neighbors)
        return self._batch_results(ids, d, cnt, include_distances, meta_db)

    # ---- radius search and near-duplicate pairs ------------------------------------------------
    def _check_radius_possible(self):
        if not isinstance(self.annoy_index, AnnoyIndex):
            raise ValueError(RADIUS_SHARDS_REFUSAL)

    def _radius_results(self, lists, counts, include_distances, meta_db, num_neighbors):
        """_result_rows for the variable-length lists of AnnoyIndex.exact_radius, cut to num_neighbors when given."""
        if num_neighbors is not None:
            lists = [(ids[:num_neighbors], d[:num_neighbors]) for ids, d in lists]
        return self._result_rows(lists, counts, include_distances, meta_db)

    def exact_radius_nn(self, radius, num_neighbors=None, include_distances=True, meta_db=False, restriction=None):
        """exact_search_nn's list for query_sample with as many results as the index has samples, cut after the last one
        whose distance is <= radius (and to num_neighbors when given); ValueError where exact_search_nn raises."""
        self._check_radius_possible()
        self._check_restriction(restriction, None)
        lists, counts = self.annoy_index.exact_radius(radius, Q=np.array([self.query_sample], dtype=np.float64),
                                                      restriction=restriction.handle if restriction is not None else None)
        res = self._radius_results(lists, counts, include_distances, meta_db, num_neighbors)[0]
        if isinstance(res, Exception):
            raise res
        return res

    def exact_radius_nn_batch(self, batch, radius, include_distances=True, meta_db=False, restriction=None, query_groups=None,
                              num_neighbors=None):
        """exact_radius_nn for every query of `batch` (a QueryBatch, or a list of EXTERNAL ids of indexed samples, searched
        by item): a list of result tuples, in query order; a ValueError instance where the reference would raise.  Under a
        restriction with groups a by-item query carries its own sample's group unless query_groups says otherwise."""
        self._check_radius_possible()
        self._check_restriction(restriction, query_groups)
        handle = restriction.handle if restriction is not None else None
        if isinstance(batch, QueryBatch):
            self._check_batch(batch)
            lists, counts = self.annoy_index.exact_radius(radius, Q=batch.rows64, restriction=handle, query_groups=query_groups)
        else:
            internal = self._internal_ids(batch)
            if restriction is not None and query_groups is None:
                query_groups = restriction.own_groups(internal)
            lists, counts = self.annoy_index.exact_radius(radius, items=np.array(internal, np.int32), restriction=handle,
                                                          query_groups=query_groups)
        return self._radius_results(lists, counts, include_distances, meta_db, num_neighbors)

    def _internal_ids(self, query_ids):
        internal = []
        for query_id in query_ids:
            if query_id not in self.internal_id_map:
                raise ValueError("Querying sample id " + str(query_id)
                                 + " is not possible because no internal id is mapped to that "
                                 + "sample id. Likely no sample with that id was included "
                                 + "in the index.")
            internal.append(self.internal_id_map[query_id])
        return internal

    def sample_pairs(self, radius, restriction=None, groups=True):
        """Every unordered pair of indexed samples within `radius` of each other: a list of (idA, idB, distance), EXTERNAL
        ids with idA < idB, in sort_pairs order (NaN pairs -- two rows closer than fp64 can tell -- first).  One radius
        search by item over all items, every query bounded to the ids above its own.  restriction: only its allowed samples
        take part; groups: with a restriction made with groups, never pair two samples of one group."""
        self._check_radius_possible()
        self._check_restriction(restriction, None)
        n = self.annoy_index.get_n_items()
        items = np.arange(n, dtype=np.int32)
        if restriction is not None and restriction.allow is not None:
            items = items[restriction.allow]
        own = restriction.own_groups(items) if restriction is not None and groups else None
        lists, _ = self.annoy_index.exact_radius(radius, items=items, after=items, query_groups=own,
                                                 restriction=restriction.handle if restriction is not None else None)
        inv = self._inverse_map()
        pairs = []
        for i, (ids, d) in zip(items.tolist(), lists):
            a = inv[i]
            for j, dist in zip(ids.tolist(), d.tolist()):
                b = inv[j]
                pairs.append((min(a, b), max(a, b), dist))
        return sort_pairs(pairs)

    # ---- spherical k-means over the index rows ---------------------------------------------------
    def cluster_samples(self, k=None, seed=0, init_ids=None, max_iterations=100, restriction=None):
        """A partition of the indexed samples into k groups by angular distance in the hashed space: spherical k-means on the
        GPU (AnnoyIndex.kmeans), bit-reproducible.  The first centroids are the rows of init_ids (EXTERNAL ids, distinct; k is
        then their number) or of cluster_seed_items(eligible, k, seed).  restriction: a SearchRestriction made without groups;
        only its allowed samples are partitioned.  Returns a SearchClusters."""
        self._device_index(CLUSTER_SHARDS_REFUSAL)
        self._check_restriction(restriction, None)
        if restriction is not None and restriction.item_group is not None:
            raise ValueError("cluster takes a restriction without groups (within / without only)")
        n = self.annoy_index.get_n_items()
        allow = restriction.allow if restriction is not None else None
        eligible = list(range(n)) if allow is None else np.nonzero(allow)[0].tolist()
        if init_ids is not None:
            init_ids = list(init_ids)
            if k is not None and k != len(init_ids):
                raise ValueError("cluster: k = %d, but %d first centroids are named" % (k, len(init_ids)))
            k = len(init_ids)
            seeds = self._internal_ids(init_ids)
        else:
            if k is None:
                raise ValueError("cluster needs k or init_ids")
            seeds = None
        if not 1 <= k <= min(LABELS_MAX, len(eligible)):
            raise ValueError(cluster_max_refusal(k, len(eligible)))
        if k * n > CLUSTER_MAX_VALUES:
            raise ValueError("cluster: k * samples = %d is above 2^29 = %d, the distances one pass keeps on the GPU"
                             % (k * n, CLUSTER_MAX_VALUES))
        if seeds is None:
            seeds = cluster_seed_items(eligible, k, seed)
        out = self.annoy_index.kmeans(seeds, max_iterations, restriction=restriction.handle if restriction is not None else None)
        inv = self._inverse_map()
        assign, dist = out["assign"], out["dist"]
        members = [[] for _ in range(k)]
        samples = []
        for i, (j, d) in enumerate(zip(assign.tolist(), dist.tolist())):
            if j >= 0:
                members[j].append(inv[i])
                samples.append((inv[i], j, d))
        table = cluster_table(assign, dist, k)
        return SearchClusters([(cluster_label(j), members[j]) for j in range(k)], [t[0] for t in table], [t[1] for t in table],
                              [None if t[2] is None else inv[t[2]] for t in table], samples, out["iterations"], out["converged"],
                              self.annoy_index.kmeans_stats())

    # ---- principal axes of the index rows ---------------------------------------------------------
    def principal_axes(self, p=10, extra=8, center=True, seed=0, tol=1e-9, max_iterations=500, restriction=None):
        """The p leading principal axes of the unit-scaled rows of the indexed samples, fitted on the GPU (AnnoyIndex.pca),
        bit-reproducible.  restriction: a SearchRestriction made without groups; only its allowed samples are fitted (every
        sample can still be placed: pca_samples, pca_coordinates).  Returns a SearchPCA."""
        self._device_index(PCA_SHARDS_REFUSAL)
        self._check_restriction(restriction, None)
        if restriction is not None and restriction.item_group is not None:
            raise ValueError("pca takes a restriction without groups (within / without only)")
        if not 1 <= p <= PCA_MAX_COMPONENTS or extra < 0 or p + extra > PCA_MAX_BLOCK:
            raise ValueError(pca_width_refusal(p, extra))
        out = self.annoy_index.pca(p, extra, center, seed, tol, max_iterations,
                                   restriction=restriction.handle if restriction is not None else None)
        return SearchPCA(out["axes"], out["mean"], out["values"], out["iterations"], out["converged"], out["fitted"],
                         out["total_variance"], self.annoy_index.pca_stats())

    def pca_coordinates(self, pca, queries):
        """The coordinates (float64 [nq, p]) on the axes of `pca` of a QueryBatch (queries_from_intropolis), of fp64 query
        vectors [nq, dim], or of a list of INTERNAL ids."""
        self._device_index(PCA_SHARDS_REFUSAL)
        if isinstance(queries, QueryBatch):
            self._check_batch(queries)
            return self.annoy_index.pca_project(pca.axes, pca.mean)
        source, queries = vectors_or_items(queries)
        nq = len(queries)
        coords = np.zeros((nq, pca.axes.shape[0]), np.float64)
        step = max(1024, PCA_CALL_VALUES // self.annoy_index.f)   # queries of one call: its staging stays modest
        chunked_call(lambda q0, q1: (self.annoy_index.pca_project(pca.axes, pca.mean, **{source: queries[q0:q1]}),), nq, step, (coords,))
        return coords

    def pca_samples(self, pca):
        """Places every indexed sample on the axes of `pca`: fills pca.samples (EXTERNAL ids in ascending internal id) and
        pca.coords, and returns pca."""
        n = self.annoy_index.get_n_items()
        inv = self._inverse_map()
        pca.coords = self.pca_coordinates(pca, range(n))
        pca.samples = [inv[i] for i in range(n)]
        return pca

    def search_recall(self, queries, num_neighbors, trees, search_ks):
        """The recall of the approximate search against the exact one for every (tree count, search_k) of a grid, from this
        one index (AnnoyIndex.recall_sweep).  queries: a QueryBatch (queries_from_intropolis) or a list of
        INTERNAL ids.  trees / search_ks: strictly ascending positive integers, at most 64 each, trees at most the index's
        tree count; num_neighbors at most 256.  Returns a SearchRecall."""
        self._device_index(TREES_SHARDS_REFUSAL)
        trees, search_ks = [int(t) for t in trees], [int(s) for s in search_ks]
        if isinstance(queries, QueryBatch):
            self._check_batch(queries)
            out = self.annoy_index.recall_sweep(num_neighbors, trees, search_ks)
        else:
            out = self.annoy_index.recall_sweep(num_neighbors, trees, search_ks, items=np.array(list(queries), np.int32))
        return SearchRecall(trees, search_ks, out)

    def _group_labels(self, groups, maximum, refusal):
        """(names, item_label int32 [n_items], n_labels) of `groups`, [(label, [EXTERNAL ids])]: 1 to `maximum` labels, else
        ValueError(refusal(their number)); an id in two labels or outside the index is restriction_arrays' ValueError."""
        groups = list(groups)
        if not 1 <= len(groups) <= maximum:
            raise ValueError(refusal(len(groups)))
        _, item_label, n_labels = restriction_arrays(self.internal_id_map, self.annoy_index.get_n_items(), groups=groups)
        return [label for label, _ in groups], item_label, n_labels

    def label_separation(self, queries, groups, restriction=None, query_groups=None):
        """For every query and every label of `groups` the sum of the angular distances, in the hashed space, to the samples
        that carry the label, and their number -- from one scan of the index on the GPU (AnnoyIndex.label_sums; DESIGN.md 8,
        N13).  queries: a QueryBatch (queries_from_intropolis), fp64 query vectors [nq, dim], or a list of INTERNAL ids -- such
        a query is not counted among its own label's samples, and its own label is what label_summary / label_map compare
        with.  groups: [(label, [EXTERNAL ids])] as parse_groups_file returns it, at most 4096 labels; an id in two labels or
        outside the index is restriction_arrays' ValueError.  restriction / query_groups: as the *_batch searches; a by-item
        query under a restriction with groups carries its own sample's group unless query_groups says otherwise.  Returns a
        SearchLabels."""
        self._device_index(LABELS_SHARDS_REFUSAL)
        names, item_label, n_labels = self._group_labels(groups, LABELS_MAX, labels_max_refusal)
        self._check_restriction(restriction, query_groups)
        handle = restriction.handle if restriction is not None else None
        stats = {name: kind() for name, kind in LABEL_SUMS_STATS}

        def scan(**source):
            out = self.annoy_index.label_sums(item_label, n_labels, restriction=handle, **source)
            accumulate_stats(stats, self.annoy_index.label_sums_stats(), maxima=("scan_eps",))
            return out
        if isinstance(queries, QueryBatch):
            self._check_batch(queries)
            sums, counts = scan(query_groups=query_groups)
            return SearchLabels(names, item_label, sums, counts, None, stats)
        source, queries = vectors_or_items(queries)
        if source == "items" and restriction is not None and query_groups is None:
            query_groups = restriction.own_groups(queries)
        if query_groups is not None:
            query_groups = np.ascontiguousarray(query_groups, dtype=np.int32)
        nq = len(queries)
        sums, counts = np.zeros((nq, n_labels), np.uint64), np.zeros((nq, n_labels), np.int32)
        step = max(1024, LABELS_CALL_CELLS // n_labels)        # queries of one call: its outputs stay modest
        chunked_call(lambda q0, q1: scan(query_groups=None if query_groups is None else query_groups[q0:q1],
                                         **{source: queries[q0:q1]}), nq, step, (sums, counts))
        return SearchLabels(names, item_label, sums, counts, item_label[queries] if source == "items" else None, stats)

    def label_mixture(self, queries, groups, restriction=None, tol=1e-9, max_sweeps=10000):
        """Every query as a non-negative combination of the centroids of the labels of `groups`, fitted on the GPU
        (AnnoyIndex.mixture).  queries: a QueryBatch (queries_from_intropolis), fp64 query vectors [nq, dim],
        or a list of INTERNAL ids -- such a query is left out of its own label's centroid.  groups: [(label, [EXTERNAL ids])]
        as parse_groups_file returns it, at most 128 labels; an id in two labels or outside the index is restriction_arrays'
        ValueError.  restriction: an allow-list only (the library refuses one made with groups).  Returns a SearchMixture."""
        self._device_index(MIXTURE_SHARDS_REFUSAL)
        names, item_label, n_labels = self._group_labels(groups, MIXTURE_LABELS_MAX, mixture_max_refusal)
        self._check_restriction(restriction, None)
        handle = restriction.handle if restriction is not None else None
        stats = {name: kind() for name, kind in MIXTURE_STATS}

        def fit(**source):
            out = self.annoy_index.mixture(item_label, n_labels, restriction=handle, tol=tol, max_sweeps=max_sweeps, **source)
            accumulate_stats(stats, self.annoy_index.mixture_stats(), maxima=("max_sweeps",))
            return out
        if isinstance(queries, QueryBatch):
            self._check_batch(queries)
            weights, info, active = fit()
            return SearchMixture(names, item_label, weights, info, active, None, stats)
        source, queries = vectors_or_items(queries)
        nq = len(queries)
        weights, info = np.zeros((nq, n_labels), np.float64), np.zeros((nq, 4), np.float64)
        active = np.zeros((nq, n_labels), bool)
        step = max(1024, MIXTURE_CALL_CELLS // n_labels)       # queries of one call: its outputs stay modest
        chunked_call(lambda q0, q1: fit(**{source: queries[q0:q1]}), nq, step, (weights, info, active))
        return SearchMixture(names, item_label, weights, info, active, item_label[queries] if source == "items" else None, stats)

    def hashing_sweep(self, query_ids, num_neighbors, dims, junction_file, n_trees=None, search_k=None):
        """What every width of `dims` costs in neighbours and in norm distortion, from this one index.
        query_ids: EXTERNAL sample ids of the index; the truth of a query is its unhashed neighbours (unhashed_search_member_n_
        batch of num_neighbors + 1, the query dropped).  For every D the index's items are hashed again at width D on the GPU,
        straight from the junction store (AnnoyIndex.add_items_from_store: the weights of <basename>.jw.mor, the line hashes
        of `junction_file`, the intropolis file the index was made from), and searched exactly; with n_trees also through a
        forest of that many trees, search_k morna's default 100 when not given.  The population is the index's items at every
        D.  Returns a SearchHashing.  ValueError on an index of row shards, for an unknown id, or when the file's line count
        is not the store's; IOError without the store or its weights."""
        from .junctions import line_hashes
        if not isinstance(self.annoy_index, AnnoyIndex):
            raise ValueError(HASHING_SHARDS_REFUSAL)
        r = int(num_neighbors)
        dims = [int(d) for d in dims]
        query_ids = list(query_ids)
        truth_lists = self.unhashed_search_member_n_batch(query_ids, r + 1)       # (checks the ids)
        store, _ = self.unhashed_store()
        population = self._unhashed_population()
        items = np.array([self.internal_id_map[q] for q in query_ids], np.int32)
        truth = [drop_query(t[0], t[1], me, r) for t, me in zip(truth_lists, items.tolist())]
        line_hash = line_hashes(junction_file, store.n_lines, self.annoy_index)
        pp = store.row_norms(population)
        if search_k is None:
            search_k = HASHING_SEARCH_K
        exact, approx, norm_stats, kernel_ms = [], [], [], []
        for d in dims:
            handle = AnnoyIndex(d, metric="angular", device=self._device)
            try:
                handle.add_items_from_store(store, population, line_hash)
                kernel_ms.append(store.hash_rows_stats()["kernel_ms"])
                norm_stats.append(norm_ratio_stats(handle.get_norms2(), pp))
                ids, dist, cnt = handle.exact_search_by_item_batch(items, r + 1)
                if (cnt < 0).any():
                    raise ValueError("math domain error (the exact search at %d features)" % d)
                exact.append([drop_query(ids[q, :int(cnt[q])], dist[q, :int(cnt[q])], me, r) for q, me in enumerate(items.tolist())])
                if n_trees is not None:
                    handle.build(int(n_trees))
                    ids, dist, cnt = handle.get_nns_by_item_batch(items, r + 1, int(search_k))
                    approx.append([drop_query(ids[q, :max(int(cnt[q]), 0)], dist[q, :max(int(cnt[q]), 0)], me, r)
                                   for q, me in enumerate(items.tolist())])
            finally:
                handle.__del__()              # the rows of one width are freed before the next is made
        tables = [hashing_rows(dims, truth[q], [e[q] for e in exact], [a[q] for a in approx] if n_trees is not None else None)
                  for q in range(len(query_ids))]
        return SearchHashing(dims, tables, norm_stats, kernel_ms)

    def search_member_n_batch(self, query_ids, num_neighbors, search_k, include_distances=True, meta_db=False, restriction=None,
                              query_groups=None, n_trees=None):
        """search_member_n for several indexed sample ids, searched together (get_nns_by_item_batch); an unknown id fails
        before any search, with search_member_n's message.  Returns (internal ids, list of result tuples).  restriction:
        MornaSearch.restriction; query_groups None under a restriction with groups: every query carries its own sample's
        group."""
        self._device_index()
        internal = self._internal_ids(query_ids)
        self._check_restriction(restriction, query_groups)
        self._check_trees(n_trees, restriction)
        if n_trees is not None:
            ids, d, cnt = self.annoy_index.get_nns_by_item_batch(np.array(internal, np.int32), num_neighbors, search_k,
                                                                 n_trees=n_trees)
            return internal, self._batch_results(ids, d, cnt, include_distances, meta_db)
        if restriction is not None:
            if query_groups is None:
                query_groups = restriction.own_groups(internal)
            ids, d, cnt = self.annoy_index.get_nns_restricted(
                restriction.handle, num_neighbors, self._restricted_search_k(restriction, num_neighbors, search_k),
                items=np.array(internal, np.int32), query_groups=query_groups)
            return internal, self._batch_results(ids, d, cnt, include_distances, meta_db)
        ids, d, cnt = self.annoy_index.get_nns_by_item_batch(np.array(internal, np.int32), num_neighbors, search_k)
        return internal, self._batch_results(ids, d, cnt, include_distances, meta_db)

    # ---- junctions of the results (morna.py:1486-1569) ----------------------------------------------------------
    def junction_store(self):
        """<basename>.junc.mor, loaded on first use."""
        if self._junction_store is None:
            from .junctions import STORE_SUFFIX, JunctionStore
            self._device_index()
            path = self.basename + STORE_SUFFIX
            if not os.path.exists(path):
                raise IOError("%s not found: this index has no junction store; build it with `morna index "
                              "--junction-store`" % path)
            self._junction_store = JunctionStore.load(path, device=self._device)
        return self._junction_store

    def result_sample_ids(self, result_list):
        """External sample ids of a list of internal ids (inverse_lookup, morna.py:1501-1504)."""
        inv = self._inverse_map()
        return [inv[int(i)] for i in result_list]

    def retain_junctions(self, result_lists, frequency_filter, coverage_filter):
        """The junctions to hand to the aligner for each list of results (internal ids in rank order, as search_nn
        returns them; at most 64 per list): those found in at least ceil(frequency_filter * len(list)) of the list's
        samples, or covered at least coverage_filter times in one of them (morna.py:1539-1569).  All lists are answered
        in one call on the GPU.  Returns one junctions.Retained per list: lines, found_in, coverages."""
        store = self.junction_store()
        return store.retain([self.result_sample_ids(lst) for lst in result_lists], frequency_filter, coverage_filter)

    def junction_recovery(self, result_lists, truth, coverage_grid, truth_min_coverage=1):
        """The recovery histograms (junctions.JunctionStore.recovery) of every list of results (internal
        ids in rank order, as retain_junctions takes them).  truth: per list, either an internal id -- the truth is that
        sample's own junctions covered at least truth_min_coverage times -- or an array of line numbers of the indexed
        file.  Returns int64 [len(result_lists)][2][65][len(coverage_grid) + 1] for junctions.recovery_rows."""
        store = self.junction_store()
        lists = [self.result_sample_ids(lst) for lst in result_lists]
        truth = list(truth)
        if all(np.ndim(t) == 0 for t in truth):
            return store.recovery_by_sample(lists, self.result_sample_ids(truth), coverage_grid, truth_min_coverage)
        return store.recovery(lists, truth, coverage_grid)

    def junction_recovery_sweep(self, result_lists, truth, coverage_grid, prefixes, truth_min_coverage=1):
        """junction_recovery for several lengths of every list from one pass (junctions.JunctionStore.recovery_sweep;
        DESIGN.md 8, N7): prefixes ascending, 1 to 64, at most 8.  Returns int64 [len(result_lists)][len(prefixes)][2][65]
        [len(coverage_grid) + 1]; [q][i] is the histogram of list q cut to its first prefixes[i] results."""
        store = self.junction_store()
        lists = [self.result_sample_ids(lst) for lst in result_lists]
        truth = list(truth)
        if all(np.ndim(t) == 0 for t in truth):
            return store.recovery_sweep_by_sample(lists, self.result_sample_ids(truth), coverage_grid, prefixes, truth_min_coverage)
        return store.recovery_sweep(lists, truth, coverage_grid, prefixes)

    # ---- pooled samples as queries (create_supersample.py of the reference's tests/) -------------------
    def pool_samples(self, groups):
        """One junctions.Pooled per group of external sample ids (junctions.JunctionStore.pool): the summed coverage of
        every junction line a sample of the group holds, all groups in one call on the GPU."""
        return self.junction_store().pool(groups)

    @staticmethod
    def _check_pooled_coverages(pooled, labels):
        """The query paths take int32 coverages: ValueError naming the group and the line for a sum that does not fit."""
        for label, r in zip(labels, pooled):
            sums = np.asarray(r.sums, np.int64)
            bad = np.nonzero((sums > 2**31 - 1) | (sums < -2**31))[0]
            if len(bad):
                raise ValueError("group %s: the summed coverage of line %d is %d, which does not fit 32 bits (2^31 - 1 at the "
                                 "most): a query takes int32 coverages; `morna supersample` writes such a group's file"
                                 % (label, int(r.lines[bad[0]]), int(sums[bad[0]])))

    def _queries_from_rows(self, rows, junction_file):
        """(lines ascending, integer coverages that fit int32) lists as queries of the hashed searches: for list g the
        vector update_query over its lines (key "chrom start end" of that line of `junction_file`, the (gzipped) intropolis
        file the index was made from; its coverage) and finalize_query would make -- bit for bit the row of an intropolis
        file that lists the lists as samples with those coverages.  ValueError when the file's line count is not the
        store's."""
        from .index import ParsedLines
        n_lines = self.junction_store().n_lines
        parsed = ParsedLines(junction_file, sample_count=1, sample_threshold=0)
        if parsed.lines_read != n_lines:
            raise ValueError("%s has %d lines, the junction store has %d: it is not the file that was indexed"
                             % (junction_file, parsed.lines_read, n_lines))
        a = parsed.arrays()
        # list-major (line, coverage) lists -> line-major rows of (list, coverage); a list's lines ascend, so file order is kept
        line = np.concatenate([np.asarray(l, np.int64) for l, _ in rows] + [np.zeros(0, np.int64)])
        group = np.concatenate([np.full(len(l), g, np.int64) for g, (l, _) in enumerate(rows)] + [np.zeros(0, np.int64)])
        cov = np.concatenate([np.asarray(c, np.int64) for _, c in rows] + [np.zeros(0, np.int64)])
        order = np.lexsort((group, line))
        line, group, cov = line[order], group[order], cov[order]
        held, per_line = np.unique(line, return_counts=True)
        row_ptr = np.zeros(len(held) + 1, np.int64)
        np.cumsum(per_line, out=row_ptr[1:])
        key_off, key_bytes = np.asarray(a["key_off"]), np.asarray(a["key_bytes"])
        key_len = key_off[held + 1] - key_off[held]
        out_off = np.zeros(len(held) + 1, np.int64)
        np.cumsum(key_len, out=out_off[1:])
        take = np.repeat(key_off[held] - out_off[:-1], key_len) + np.arange(int(out_off[-1]), dtype=np.int64)
        prep = dict(key_bytes=key_bytes[take], key_off=out_off, row_ptr=row_ptr, ids=group, cov=cov,
                    idf=np.zeros(len(held), np.float64), ext_ids=np.arange(len(rows), dtype=np.int64))
        lines = ParsedLines.from_arrays(prep, self.sample_count)
        return self._batch_from_terms(lines.query_terms(self._vocab(), self.sample_count))

    def _unhashed_terms_from_rows(self, rows):
        """(lines ascending, integer coverages that fit int32) lists as the term lists of unhashed_search_nn_batch, the
        lines of weight 0 left out as junctions.query_terms leaves them out."""
        _, w = self.unhashed_store()
        terms = []
        for l, c in rows:
            keep = np.asarray(w)[np.asarray(l, np.int64)] != 0.0
            terms.append((np.asarray(l, np.int32)[keep], np.asarray(c, np.int64)[keep].astype(np.int32)))
        return terms

    def queries_from_pooled(self, pooled, labels, junction_file):
        """The groups of pool_samples as queries of the hashed searches: for group g the vector update_query over the
        lines it holds (key "chrom start end" of that line of `junction_file`, the (gzipped) intropolis file the index
        was made from; the group's summed coverage) and finalize_query would make -- bit for bit the row of an intropolis
        file that lists the groups as samples with those sums.  Returns a QueryBatch whose query q is group q; `labels`
        name the groups in messages.  ValueError when the file's line count is not the store's, or a sum does not fit
        int32."""
        self._check_batch_possible()
        pooled, labels = list(pooled), list(labels)
        self._check_pooled_coverages(pooled, labels)
        return self._queries_from_rows([(r.lines, r.sums) for r in pooled], junction_file)

    def unhashed_terms_from_pooled(self, pooled, labels):
        """The groups of pool_samples as the term lists of unhashed_search_nn_batch: (lines ascending, coverages) per
        group, the lines of weight 0 left out as junctions.query_terms leaves them out."""
        pooled, labels = list(pooled), list(labels)
        self._check_pooled_coverages(pooled, labels)
        return self._unhashed_terms_from_rows([(r.lines, r.sums) for r in pooled])

    # ---- store rows at a fraction of their depth as queries -----------------------------------------------
    def thin_samples(self, sample_ids, keep, seed):
        """One junctions.Thinned per job (external sample id, keep threshold in [0, 2^32]) (junctions.JunctionStore.thin):
        the sample's row with every read kept with probability keep / 2^32, all jobs in one call on the GPU."""
        return self.junction_store().thin(sample_ids, keep, seed)

    def queries_from_thinned(self, thinned, junction_file):
        """The rows of thin_samples as queries of the hashed searches: bit for bit the rows of an intropolis file that lists
        every job as a sample of its own with the thinned coverages.  Returns a QueryBatch whose query q is job q."""
        self._check_batch_possible()
        return self._queries_from_rows([(r.lines, r.cov) for r in thinned], junction_file)

    def unhashed_terms_from_thinned(self, thinned):
        """The rows of thin_samples as the term lists of unhashed_search_nn_batch."""
        return self._unhashed_terms_from_rows([(r.lines, r.cov) for r in thinned])

    # ---- unhashed TF-IDF search: no counterpart the reference finished -------------------------
    def unhashed_store(self):
        """The junction store with the line weights of <basename>.jw.mor set, and those weights; on first use."""
        if getattr(self, "_unhashed_weights", None) is None:
            from .junctions import WEIGHTS_SUFFIX, load_weights
            store = self.junction_store()
            path = self.basename + WEIGHTS_SUFFIX
            if not os.path.exists(path):
                raise IOError("%s not found: --unhashed needs the line weights `morna index --junction-store` writes next "
                              "to the junction store. They are not written when a junction repeats in the indexed file: "
                              "the unhashed search is defined for files without repeated junctions" % path)
            w, _, _ = load_weights(path, store.n_lines)
            store.set_weights(w)
            self._unhashed_weights = w
        return self.junction_store(), self._unhashed_weights

    def _unhashed_population(self):
        """The items of the index as external sample ids, in internal-id order."""
        inv = self._inverse_map()
        return np.array([inv[i] for i in range(len(inv))], np.int64)

    @staticmethod
    def _unhashed_ids(ids, restriction):
        """Positions in a narrowed population back to internal ids (-1 stays -1)."""
        if restriction is None or restriction.allow is None:
            return ids
        at = np.nonzero(restriction.allow)[0].astype(np.int32)
        if len(at) == 0:
            return np.full_like(ids, -1)
        return np.where(ids >= 0, at[np.clip(ids, 0, len(at) - 1)], -1).astype(np.int32)

    def unhashed_search_member_n_batch(self, query_ids, num_neighbors, include_distances=True, meta_db=False, restriction=None):
        """The unhashed neighbours of several indexed sample ids: a list of result tuples in query order, as
        exact_search_nn_batch returns them (internal ids); an unknown id fails with search_member_n's message."""
        self._internal_ids(query_ids)
        store, _ = self.unhashed_store()
        ids, d, cnt = store.nearest_by_sample(self._unhashed_population_of(restriction), [int(q) for q in query_ids], num_neighbors)
        ids = self._unhashed_ids(ids, restriction)
        return self._batch_results(ids, d, cnt, include_distances, meta_db)

    def unhashed_search_nn_batch(self, term_lists, num_neighbors, include_distances=True, meta_db=False, restriction=None):
        """The unhashed neighbours of queries given as (lines ascending, coverages) pairs over the lines of the indexed
        file (junctions.query_terms / intropolis_query_terms): a list of result tuples in query order."""
        store, _ = self.unhashed_store()
        ids, d, cnt = store.nearest(self._unhashed_population_of(restriction), term_lists, num_neighbors)
        ids = self._unhashed_ids(ids, restriction)
        return self._batch_results(ids, d, cnt, include_distances, meta_db)

    # ---- the junctions behind a query and each result: no counterpart in the reference -----------
    def explain_results(self, result_lists, queries, top=10):
        """For every query and every result of its list (internal ids in rank order, as retain_junctions takes them; at most
        1024 per list) the decomposition of their unhashed cosine (junctions.JunctionStore.explain): one list of
        junctions.Explained per query.  queries: internal ids, or the (lines ascending, coverages) term lists of
        unhashed_search_nn_batch.  All pairs in one call on the GPU."""
        store, _ = self.unhashed_store()
        lists = [self.result_sample_ids(lst) for lst in result_lists]
        queries = list(queries)
        if all(np.ndim(q) == 0 for q in queries):
            return store.explain_by_sample(self.result_sample_ids(queries), lists, top)
        return store.explain(queries, lists, top)

    def search_member_n(self, query_id, num_neighbors, search_k, include_distances=True, meta_db=False, n_trees=None):
        """Neighbours of an indexed sample (morna.py:733-787); n_trees: as search_nn."""
        self._check_trees(n_trees)
        print("querying by sample id " + str(query_id))
        internal_id = self._internal_ids([query_id])[0]
        print("this is internal id " + str(internal_id))
        if n_trees is not None:
            results = self.annoy_index.get_nns_by_item(internal_id, num_neighbors, search_k, include_distances, n_trees=n_trees)
            return self._with_meta(results if include_distances else (results,), meta_db)
        if include_distances:
            results = self.annoy_index.get_nns_by_item(internal_id, num_neighbors, search_k, include_distances)
        else:
            results = (self.annoy_index.get_nns_by_item(internal_id, num_neighbors, search_k, include_distances),)
        return self._with_meta(results, meta_db)
