"""The text of the host program's -d / -D and -i / -S files, rebuilt from main
output records and a definition of the stage (the Python references or the
*_host functions): shared by the CLI tests of tests/test_gpu_barcode.py,
tests/test_gpu_scan.py and tests/test_gpu_cli_stages.py."""
from __future__ import annotations

import ccsx_amd as cx

DEMUX_HEADER = "#name\tlen\tbc0\tstrand0\tscore0\tsecond0\tend0\tbc1\tstrand1\tscore1\tsecond1\tend1\tcl\tcr\tcalled0\tcalled1\tassigned\treason"
SCAN_HEADER = "#name\tlen\tadapter\tstrand\tstart\tend\tscore\talen"


def records(main: str, fastq: bool) -> list:
    """[(header without its first character, bases, qualities or None)] of a main output."""
    lines = main.split("\n")[:-1]
    step = 4 if fastq else 2
    return [(lines[k][1:], lines[k + 1], lines[k + 3] if fastq else None) for k in range(0, len(lines), step)]


def demux_files(recs, barcodes, names, fastq: bool, score, call, window: int = 96) -> tuple:
    """(the -d file, the -D file, [(result, call)] per record) for main output
    records; score(barcodes, ccs, window) and call(result, lens, n) define the stage."""
    lens = [len(b) for b in barcodes]
    want_d, want_t, rows = "", [DEMUX_HEADER], []
    for head, seq, qual in recs:
        r = score(barcodes, seq.encode(), window)
        c = call(r, lens, len(seq))
        cl, cr, called, assigned, reason = c
        rows.append((r, c))
        row = [head.split()[0], str(len(seq))]
        for e in r:
            # (the runner-up's score: "." for a set of one barcode, which has none)
            row += [names[e[0] >> 1], "-" if e[0] & 1 else "+", str(e[1]), "." if e[4] < 0 else str(e[3]), str(e[2])]
        row += [str(cl), str(cr), str(int(called[0])), str(int(called[1])), str(int(assigned)), cx.BC_REASONS[reason]]
        want_t.append("\t".join(row))
        if not assigned:
            continue
        h = f"{head} bc={names[r[0][0] >> 1]}--{names[r[1][0] >> 1]} bs={r[0][1]},{r[1][1]} bx={cl},{cr}"
        trimmed = seq[cl:len(seq) - cr]
        want_d += f"@{h}\n{trimmed}\n+\n{qual[cl:len(seq) - cr]}\n" if fastq else f">{h}\n{trimmed}\n"
    return want_d, "\n".join(want_t) + "\n", rows


def scan_files(recs, adapters, names, fastq: bool, hits, cut) -> tuple:
    """(the -i file, the -S file, [hits] per record) for main output records;
    hits(adapters, ccs) and cut(hits, n) define the stage."""
    want_t, want_p, found = [SCAN_HEADER], "", []
    for head, seq, qual in recs:
        name = head.split()[0]
        hs = hits(adapters, seq.encode())
        found.append(hs)
        for a, o, s, e, score in hs:
            want_t.append("\t".join([name, str(len(seq)), names[a], "-" if o else "+", str(s), str(e), str(score),
                                     str(len(adapters[a]))]))
        flank = lambda x: "." if x < 0 else names[hs[x][0]] + ("-" if hs[x][1] else "+")  # noqa: E731
        for b, e, left, right in cut(hs, len(seq)):
            h = f"{name}/{b}_{e} la={flank(left)} ra={flank(right)}"
            want_p += f"@{h}\n{seq[b:e]}\n+\n{qual[b:e]}\n" if fastq else f">{h}\n{seq[b:e]}\n"
    return "\n".join(want_t) + "\n", want_p, found
