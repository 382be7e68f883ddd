"""Compare the kernels of two assembly listings (`hipcc -S --cuda-device-only` outputs), e.g. a parent build and a refactored one.  CPU only.

    python tools/isa_diff.py old.s new.s [old_symbol=new_symbol ...] [--md]

Kernels are matched by symbol; a kernel that was renamed is given as old=new, every other symbol of old.s is looked up under its own name.  Per
kernel: (a) is the instruction text identical, (b) is the mnemonic sequence from the first to the last v_mfma line (the main loop) identical,
(c) the mnemonic histogram delta of the whole kernel (new - old), (d) how many lines outside that span differ -- and the registers, scratch, LDS
and occupancy the compiler reports behind each kernel.  Exit status 1 if a kernel is missing or a main-loop sequence differs."""
import collections
import difflib
import re
import sys

RES = ("TotalNumSgprs", "NumVgprs", "NumAgprs", "ScratchSize", "Occupancy", "LDSByteSize")


def kernels(path):
    """{symbol: ([instruction text], {resource: value})}: operands kept, comments dropped, basic-block labels renumbered per kernel."""
    out, name, cur = {}, None, None
    for line in open(path, errors="replace"):
        m = re.match(r"^(\w+):\s*(;.*)?$", line)
        if m and not line.startswith(".L"):
            name, cur = m.group(1), ([], {})
            continue
        if name is None:
            continue
        if line.startswith(".Lfunc_end"):
            out[name] = cur                      # the resource comments follow the end label
            continue
        m = re.match(r"^; (\w+): (\d+)", line)
        if m and m.group(1) in RES and name in out:
            cur[1].setdefault(m.group(1), int(m.group(2)))
            continue
        text = line.split(";")[0].strip()
        if text and not text.startswith(".") and name not in out:
            cur[0].append(re.sub(r"\.LBB\d+_", ".LBB_", text))
    return {k: v for k, v in out.items() if any(t.startswith("s_endpgm") for t in v[0])}


def mnemonics(text):
    return [t.split()[0] for t in text]


def span(text):
    idx = [i for i, t in enumerate(text) if t.startswith("v_mfma")]
    return (idx[0], idx[-1] + 1) if idx else (0, 0)


def main():
    args = [a for a in sys.argv[1:] if a != "--md"]
    md = "--md" in sys.argv
    old, new = kernels(args[0]), kernels(args[1])
    names = dict(a.split("=") for a in args[2:])
    bad = False
    if md:
        print("| kernel | text | MFMA span | histogram delta | lines differing outside the span | " + " | ".join(RES) + " |\n|---|---|---|---|---|" + "---|" * len(RES))
    for k in sorted(old):
        n = names.get(k, k)
        if n not in new:
            print(f"{k}: MISSING in {args[1]} (looked for {n})")
            bad = True
            continue
        (a, ra), (b, rb) = old[k], new[n]
        (a0, a1), (b0, b1) = span(a), span(b)
        same_span = mnemonics(a[a0:a1]) == mnemonics(b[b0:b1])
        bad |= not same_span
        ha, hb = collections.Counter(mnemonics(a)), collections.Counter(mnemonics(b))
        delta = {m: hb[m] - ha[m] for m in sorted(set(ha) | set(hb)) if hb[m] != ha[m]}
        outside = sum(1 for d in difflib.ndiff(a[:a0] + a[a1:], b[:b0] + b[b1:]) if d[0] in "+-")
        res = [f"{ra.get(r)}" if ra.get(r) == rb.get(r) else f"{ra.get(r)} -> {rb.get(r)}" for r in RES]
        cells = ["identical" if a == b else "differs", f"identical ({a1 - a0})" if same_span else f"DIFFERS ({a1 - a0} / {b1 - b0})",
                 ", ".join(f"{m} {d:+d}" for m, d in delta.items()) or "none", str(outside)]
        if md:
            print(f"| `{n}` | " + " | ".join(cells + res) + " |")
        else:
            print(f"{n}\n  text {cells[0]}; span {cells[1]}; histogram delta: {cells[2]}; outside: {cells[3]}; " + ", ".join(f"{r} {v}" for r, v in zip(RES, res)))
    extra = sorted(set(new) - {names.get(k, k) for k in old})
    if extra:
        print("only in", args[1] + ":", extra)
    sys.exit(1 if bad or extra else 0)


if __name__ == "__main__":
    main()
