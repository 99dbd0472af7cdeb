"""The per-case section of profiles/conditioning.md from the output of the conditioning tests:

    python -m pytest -m gpu -s tests/test_gpu_conditioning.py > cond.log
    python tools/conditioning_table.py cond.log profiles/conditioning.md

Every `COND | case | output | e | err | bound | verdict` line becomes a row, wherever on its line it starts, grouped by the
case's kernel; the other `COND |` lines (the derived bounds: constant group, integer sums) are listed after their group.
Everything in the document from `## Per case` on is replaced."""
import re
import sys

ROW = re.compile(r"COND \| ([^|\n]+?) \| ([^|\n]+?) \| e (\S+) \| err (\S+) \| bound (\S+) \| (ok|FAIL)")
DERIVED = re.compile(r"COND \| ([^|\n]+?) \| ([^|\n]*? \S+) \| derived bound (\S+)")
MARK = "## Per case (MI355X `err`, CPU `e`)"


def group(case):
    w = case.split()
    return " ".join(w[:2]) if w[0] == "attention" else w[0]


def main(log, doc):
    text = open(log).read()
    groups, derived = {}, {}
    for m in ROW.finditer(text):
        groups.setdefault(group(m.group(1)), []).append(m.groups())
    for m in DERIVED.finditer(text):
        derived.setdefault(group(m.group(1)), []).append(m.groups())
    rows = sum(len(v) for v in groups.values())
    out = [MARK, "", f"{rows} rows: every (case, output) pair the tests judge.", ""]
    for g, rs in groups.items():
        out += [f"### {g}", "", "| case | output | e (CPU) | err (MI355X) | bound | |", "|---|---|---|---|---|---|"]
        out += [f"| {c.strip()} | {o} | {e} | {d} | {b} | {'' if v == 'ok' else '**miss**'} |" for c, o, e, d, b, v in rs]
        if g in derived:
            out += ["", "| derived check | measured | derived bound |", "|---|---|---|"]
            out += [f"| {c} | {what} | {b} |" for c, what, b in derived[g]]
        out.append("")
    s = open(doc).read()
    open(doc, "w").write(s[:s.index(MARK)] + "\n".join(out))
    print(f"{rows} rows in {len(groups)} groups, {sum(len(v) for v in derived.values())} derived checks")


if __name__ == "__main__":
    main(*sys.argv[1:3])
