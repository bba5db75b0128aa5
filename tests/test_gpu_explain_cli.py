"""`morna explain` on the GPU through the command line, on the cohort of test_gpu_unhashed.py: the ids
and distances are those `search` prints with the same flags, the unhashed distances those of `search --unhashed -d`, and
every printed number of a pair follows from the plain-Python restatement (explain_ref.py) fed the text lines.  -m gpu"""
import re

import numpy as np
import pytest

from explain_ref import explain_pair
from test_gpu_junctions import _write_gz, run_cli
from test_gpu_unhashed import CLUSTERS, N, cohort  # noqa: F401  (the fixture)
from test_unhashed_cpu import ref_query_terms

pytestmark = pytest.mark.gpu

_PAIR = re.compile(r"^(\d+)\.\t(.*)$")


def parse_explain(text):
    """[(query label, [pair])]: a pair is the fields of its line and "top", the fields of the lines under it."""
    out = []
    for line in text.splitlines():
        if line.startswith("# query "):
            out.append((line[len("# query "):], []))
        elif line.startswith("\t"):
            out[-1][1][-1]["top"].append(line[1:].split("\t"))
        else:
            m = _PAIR.match(line)
            assert m, line
            f = m.group(2).split("\t")
            out[-1][1].append(dict(rank=int(m.group(1)), id=int(f[0]), sample=int(f[1]), search=f[2], distance=f[3],
                                   shared=int(f[4]), shares=f[5:8], meta=f[8] if len(f) > 8 else None, top=[]))
    return out


def search_lines(text):
    """(id, distance text, metadata text or None) of every result line `search -d` wrote, block by block."""
    out, last = [], ""
    for line in text.splitlines():
        if line.startswith("# query ") or (line.startswith("querying by sample id") and not last.startswith("# query ")):
            out.append([])
        last = line
        m = _PAIR.match(line)
        if m:
            if not out:
                out.append([])
            f = m.group(2).split("\t")
            out[-1].append((int(f[0]), f[1], f[2] if len(f) > 2 else None))
    return out


def share(x):
    return "nan" if x != x else "%.6f" % x


def check_pair(pair, q_row, r_row, cohort, top, summary_only=False):
    """Every number of one printed pair against the restatement."""
    want = explain_pair(q_row[0], q_row[1], r_row[0], r_row[1], cohort["w"], top)
    assert pair["distance"] == str(want["distance"]) and pair["shared"] == want["shared"]
    nan = float("nan")
    outside_q = 1.0 - want["qq_shared"] / want["qq"] if want["qq"] > 0 else nan
    outside_r = 1.0 - want["pp_shared"] / want["pp"] if want["pp"] > 0 else nan
    carried = sum(want["terms"]) / want["pq"] if want["pq"] > 0 else nan
    assert pair["shares"] == [share(outside_q), share(outside_r), share(carried)]
    if summary_only:
        assert pair["top"] == []
        return
    q_cov = dict(zip([int(l) for l in q_row[0]], [int(c) for c in q_row[1]]))
    lines = []
    for l, t, c in zip(want["lines"], want["terms"], want["cov_r"]):
        lines.append([" ".join(cohort["lines"][l].split("\t")[:3]), str(q_cov[l]), str(c), str(float(cohort["w"][l])),
                      share(t / want["pq"])])
    assert pair["top"] == lines


@pytest.mark.parametrize("flags", [["-e"], ["--unhashed"], []], ids=["exact", "unhashed", "forest"])
def test_query_ids_against_search_and_the_restatement(cohort, flags):
    items, rows = cohort["items"], cohort["rows"]
    queries = [items[i] for i in (0, 17, 150, 299)]
    ids = ",".join(map(str, queries))
    rc, out, _ = run_cli(["explain", "-x", cohort["base"], "--junction-file", cohort["src"], "--query-ids", ids, "-r", "6", "--top", "4"]
                         + flags)
    assert rc == 0
    got = parse_explain(out)
    assert [label for label, _ in got] == [str(q) for q in queries]
    rc, text, _ = run_cli(["search", "-x", cohort["base"], "--query-ids", ids, "-r", "6", "-d"] + flags)
    assert rc == 0
    rc, everything, _ = run_cli(["search", "-x", cohort["base"], "--unhashed", "--query-ids", ids, "-r", str(N), "-d"])
    assert rc == 0
    for q, (_, pairs), found, unhashed in zip(queries, got, search_lines(text), search_lines(everything)):
        assert [(p["id"], p["search"]) for p in pairs] == [(i, d) for i, d, _ in found] and len(pairs) == 6
        assert [p["rank"] for p in pairs] == list(range(1, 7))
        by_id = {i: d for i, d, _ in unhashed}
        for p in pairs:
            assert p["sample"] == items[p["id"]] and p["distance"] == by_id[p["id"]]
            check_pair(p, rows[q], rows[p["sample"]], cohort, 4)
            assert len(p["top"]) == min(4, p["shared"])


def test_one_query_id_summary_only_metadata_and_within(cohort, tmp_path):
    items, rows = cohort["items"], cohort["rows"]
    q = items[42]
    common = ["-x", cohort["base"], "-q", str(q), "-r", "5"]
    rc, full, _ = run_cli(["explain", "--junction-file", cohort["src"]] + common)
    assert rc == 0
    rc, out, _ = run_cli(["explain", "--junction-file", cohort["src"], "--summary-only", "-m"] + common)
    assert rc == 0 and "\n\t" not in out
    (label, pairs), = parse_explain(out)
    (_, full_pairs), = parse_explain(full)
    assert label == str(q) and len(pairs) == 5 and all(len(p["top"]) == min(10, p["shared"]) for p in full_pairs)
    rc, text, _ = run_cli(["search", "-d", "-m"] + common)
    assert rc == 0
    (found,) = search_lines(text)
    assert [(p["id"], p["search"], p["meta"]) for p in pairs] == found
    for p, f in zip(pairs, full_pairs):
        assert p["meta"] == str(("sample%d cluster%d\n" % ((p["sample"] - 1000) // 7, ((p["sample"] - 1000) // 7) % CLUSTERS),))
        assert {k: v for k, v in p.items() if k not in ("meta", "top")} == {k: v for k, v in f.items() if k not in ("meta", "top")}
        check_pair(p, rows[q], rows[p["sample"]], cohort, 10, summary_only=True)
        check_pair(f, rows[q], rows[f["sample"]], cohort, 10)
    # --within: the search is restricted as `search --within` restricts it
    allowed = [items[i] for i in range(0, N, 5)]
    path = tmp_path / "allowed.txt"
    path.write_text("".join("%d\n" % s for s in allowed))
    rc, out, _ = run_cli(["explain", "--junction-file", cohort["src"], "--within", str(path), "-e", "--top", "2"] + common)
    assert rc == 0
    (_, pairs), = parse_explain(out)
    rc, text, _ = run_cli(["search", "-d", "-e", "--within", str(path)] + common)
    assert rc == 0
    (found,) = search_lines(text)
    assert [(p["id"], p["search"]) for p in pairs] == [(i, d) for i, d, _ in found] and len(pairs) == 5
    for p in pairs:
        assert p["sample"] in allowed
        check_pair(p, rows[q], rows[p["sample"]], cohort, 2)


def test_against(cohort):
    items, rows, s = cohort["items"], cohort["rows"], cohort["searcher"]
    queries = [items[3], items[100]]
    listed = [items[100], items[7], items[250], items[7]]                     # a query among them, one named twice
    rc, out, _ = run_cli(["explain", "-x", cohort["base"], "--junction-file", cohort["src"], "--query-ids", ",".join(map(str, queries)),
                          "--against", ",".join(map(str, listed)), "--top", "3", "-m"])
    assert rc == 0
    got = parse_explain(out)
    assert [label for label, _ in got] == [str(q) for q in queries]
    ids, d, cnt = s.annoy_index.exact_search_by_item_batch(np.array([s.internal_id_map[q] for q in queries], np.int32), N)
    for n, (q, (_, pairs)) in enumerate(zip(queries, got)):
        exact = dict(zip(ids[n, :cnt[n]].tolist(), d[n, :cnt[n]].tolist()))
        assert [p["sample"] for p in pairs] == listed and [p["id"] for p in pairs] == [s.internal_id_map[x] for x in listed]
        for p in pairs:
            assert p["search"] == str(exact[p["id"]])
            assert p["meta"] == str(("sample%d cluster%d\n" % ((p["sample"] - 1000) // 7, ((p["sample"] - 1000) // 7) % CLUSTERS),))
            check_pair(p, rows[q], rows[p["sample"]], cohort, 3)
        assert pairs[1] == dict(pairs[3], rank=2)
    assert got[1][1][0]["distance"] == "0.0" and got[1][1][0]["shares"][:2] == ["0.000000", "0.000000"]
    with pytest.raises(ValueError) as e:
        run_cli(["explain", "-x", cohort["base"], "--junction-file", cohort["src"], "-q", str(queries[0]), "--against", "424242"])
    assert "424242" in str(e.value)


def test_outside_queries_intropolis_and_raw_stream(cohort, tmp_path):
    lines, rows, items, w = cohort["lines"], cohort["rows"], cohort["items"], cohort["w"]
    keys = [" ".join(t.split("\t")[:3]) for t in lines]
    per_sample = {70000: dict(zip(*rows[items[3]])), 70001: {5: 4, 6: 9, 900: 7}}
    qlines = []
    for j in sorted(set(per_sample[70000]) | set(per_sample[70001])):
        who = [s for s in sorted(per_sample) if j in per_sample[s]]
        qlines.append("\t".join(lines[j].split("\t")[:6] + [",".join(map(str, who)), ",".join(str(per_sample[s][j]) for s in who)]) + "\n")
    qlines.append("chrUn\t1\t2\t+\tGT\tAG\t70001\t8\n")                         # a junction the index never saw
    qpath = str(tmp_path / "queries.gz")
    _write_gz(qpath, qlines)
    first_seen = []
    for text in qlines:
        for s in text.split("\t")[6].split(","):
            if int(s) not in first_seen:
                first_seen.append(int(s))
    terms = {}
    for s in per_sample:
        t = ref_query_terms({keys[j]: c for j, c in per_sample[s].items()}, lines, w)
        terms[s] = ([j for j, _ in t], [c for _, c in t])
    for flags in (["--unhashed"], ["-e"]):
        rc, out, _ = run_cli(["explain", "-x", cohort["base"], "--junction-file", cohort["src"], "--intropolis", qpath, "-r", "4", "--top", "3"]
                             + flags)
        assert rc == 0
        got = parse_explain(out)
        assert [label for label, _ in got] == [str(s) for s in first_seen]
        rc, text, _ = run_cli(["search", "-x", cohort["base"], "--junction-file", cohort["src"], "--intropolis", qpath, "-r", "4", "-d"]
                              + flags)
        assert rc == 0
        found = dict(zip(re.findall(r"^# query (\d+)$", text, re.M), search_lines(text)))
        for label, pairs in got:
            assert [(p["id"], p["search"]) for p in pairs] == [(i, d) for i, d, _ in found[label]] and len(pairs) == 4
            for p in pairs:
                check_pair(p, terms[int(label)], rows[p["sample"]], cohort, 3)
                if flags == ["--unhashed"]:
                    assert p["distance"] == p["search"]
        assert dict(got)["70000"][0]["sample"] == items[3]
    # the second sample as a raw stream: a junction named twice is summed, an unknown one dropped
    raw = "".join("%s\t%s\t%s\t%d\n" % (tuple(keys[j].split(" ")) + (c,)) for j, c in ((5, 4), (6, 9), (900, 2), (900, 5)))
    raw += "chrUn\t1\t2\t8\n"
    rc, out, _ = run_cli(["explain", "-x", cohort["base"], "--junction-file", cohort["src"], "-f", "raw", "-e", "-r", "4", "--top", "3"],
                         stdin_text=raw)
    assert rc == 0
    (label, pairs), = parse_explain(out)
    assert label == "stdin" and pairs == dict(got)["70001"]
    rc, text, _ = run_cli(["search", "-x", cohort["base"], "-f", "raw", "-e", "-r", "4", "-d"], stdin_text=raw)
    assert rc == 0 and [(p["id"], p["search"]) for p in pairs] == [(i, d) for i, d, _ in search_lines(text)[0]]
