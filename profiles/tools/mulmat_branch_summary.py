"""Writes profiles/mulmat_branch_errors.txt from the output of `pytest -m gpu tests/test_gpu_mulmat_branches.py -q -s`:

    python -m pytest -m gpu tests/test_gpu_mulmat_branches.py -q -s > run.txt
    python profiles/tools/mulmat_branch_summary.py run.txt profiles/mulmat_branch_errors.txt <parent commit>

A header, a summary (per kernel label the worst row of either axis against the exact reference, and for the kernels that cut K the worst row
of each non-even class of K ranges), then every line the tests printed.  Every figure in the header and the summary is computed here from
those lines; nothing is typed in."""
import re
import sys

FIELD = r"token row ([0-9.e+-]+)(?: @(\d+))?, weight row ([0-9.e+-]+)(?: @(\d+))?"


def parse(line):
    sec, typ, case, shape, label, ctx, ranges, exact, orc, dist = [x.strip() for x in line.split(" | ")]
    te, ta, we, wa = re.search(FIELD, exact).groups()
    to, _, wo, _ = re.search(FIELD, orc).groups()
    td, _, wd, _ = re.search(FIELD, dist).groups()
    return dict(typ=typ, case=case, shape=shape, label=label, cls=ranges.split()[-1], fig="NMSE" if exact.startswith("NMSE") else "rel-L2",
                te=float(te), ta=ta, we=float(we), wa=wa, to=float(to), wo=float(wo), td=float(td), wd=float(wd))


def worst(rs):
    """(value, where, row) of the worst row against exact over both axes"""
    return max(((v, f"{r['typ']} {r['case']} {r['shape']} {what} @{at}", r) for r in rs
                for v, what, at in ((r["te"], "token row", r["ta"]), (r["we"], "weight row", r["wa"]))), key=lambda x: x[0])


def main(src, dst, parent):
    lines, device = [], None
    for raw in open(src):
        raw = raw.rstrip("\n").lstrip(".FEsx")           # pytest's progress marks in front of the first line of a test
        if re.match(r"^[a-z] \| ", raw):
            lines.append(raw)
        elif raw.startswith("# "):
            device = raw
    rows = [parse(l) for l in lines]
    assert device and rows, "not the -s output of tests/test_gpu_mulmat_branches.py"
    out, labels = [], list(dict.fromkeys(r["label"] for r in rows))
    for lab in labels:
        rs = [r for r in rows if r["label"] == lab]
        v, where, r = worst(rs)
        out.append(f"{lab} | per-row {r['fig']} against exact | {v:.3e} | {where} | {'within 2x' if v * 2 > (5e-4 if r['fig'] == 'NMSE' else 1e-3) else ''}")
        if re.match(r"mfma_regb_kernel<\d+,8,128>(\+combine)?$", lab) or lab == "mfma_r64_q4k_kernel<4>":
            for cls in ("ragged", "empty", "past-end"):
                cs = [x for x in rs if x["cls"] == cls]
                out.append(f"    {lab} | {cls} ranges | " + ("%.3e | %s |" % worst(cs)[:2] if cs else "- | no case of this type has such ranges |"))
    f16 = [r for r in rows if r["fig"] == "rel-L2"]
    top = worst(f16)
    mins = [r for r in f16 if r["typ"] in ("q4_1", "q5_1")]
    rest = [r for r in rows if r["typ"] not in ("q4_1", "q5_1")]
    d_tok, d_w = max(mins, key=lambda r: r["td"]), max(mins, key=lambda r: r["wd"])
    o_worst = max(mins, key=lambda r: max(r["to"], r["wo"]))
    head = f"""# tests/test_gpu_mulmat_branches.py on one MI355X, `pytest -m gpu tests/test_gpu_mulmat_branches.py -q -s` (the lines it prints), put together by
# profiles/tools/mulmat_branch_summary.py, measured on the tree of the commit that adds this file (parent {parent}).
{device}
#
# A line: section | type | case | shape | label | context | K ranges of the split-K launch and their class | worst row against exact (the float64
# product of the quantized operands) on either axis of the [N, M] output, and where | the same against the oracle (the CPU backend's arithmetic) |
# the oracle's own distance from exact.  Sections: a tile variants, b split-K range classes and both reduce paths, d groups, e in-launch combine,
# f / w the Q4_K kernels behind GGML_MI355X_R64 / R64S, g QMM_PREC_BF16.
#
# Summary, worst value per kernel label:  label | figure | worst | where | note
#   bars: per-row rel-L2 < 1e-3 on both axes against both references (default precision), per-row NMSE < 5e-4 against exact (QMM_PREC_BF16).
#   'within 2x': the worst row is within a factor of two of its bar.  Indented: the worst row over the cases whose K ranges are ragged, hold an
#   empty range, or hold a range that begins past the end of K, for the kernels that cut K.  The in-launch combine
#   takes at most four ranges, and four ranges of K >= 2048 never begin past the end: it meets ragged ranges (64-wide K-steps) and empty ones.
#   The row closest to its bar, default precision: {top[0]:.3e}, {top[2]['label']}, {top[1]}.
#   Oracle-to-exact distance, the ten types without a block minimum times a rounded sum: <= {max(max(r['td'], r['wd']) for r in rest):.3e} on any row of any case.
#   Q4_1 / Q5_1: the oracle is up to {d_tok['td']:.3e} from exact on a token row ({d_tok['typ']} {d_tok['case']}) and {d_w['wd']:.3e} on a weight row ({d_w['typ']} {d_w['case']});
#   their bar against the oracle is 1e-3 + that row's distance.  Their worst row against the oracle: {max(o_worst['to'], o_worst['wo']):.3e} ({o_worst['typ']} {o_worst['case']}); against
#   exact: {worst(mins)[0]:.3e} ({worst(mins)[1]}).
#
"""
    open(dst, "w").write(head + "\n".join(out) + "\n#\n# every line\n" + "\n".join(lines) + "\n")
    print(f"{len(lines)} lines, {len(labels)} labels -> {dst}")


if __name__ == "__main__":
    main(*sys.argv[1:4])
