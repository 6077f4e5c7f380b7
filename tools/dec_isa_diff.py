#!/usr/bin/env python3
"""Compare the decoder's generated machine code between two source trees (profiles/dec_refactor_isa.md).

    tools/dec_isa_diff.py PARENT_TREE BRANCH_TREE [--out DIR] [--reuse-parent] [--units a,b,c]

Compiles the five decoder translation units (or those named by --units, e.g. profiles/va_decide_refactor.md) for each library of __graft_entry__.VARIANTS to device assembly
(FLAGS + the variant's defines + --cuda-device-only -S), replaces __hip_cuid_<hash> (derived from the output path) and reports per unit:
"identical", or the second form: the kernels' resource metadata and the histogram of every mnemonic that is not scalar ALU / move.
A unit that differs also lists which function symbols' text differs, with their code sizes; in a unit of many kernels (tu_train: 71
symbols) the second form is judged per kernel: equal metadata, and equal counts of memory, MFMA and barrier instructions in every kernel
whose text differs (profiles/r21_train_ops_split.md).
Exit status 0 when every unit is identical or passes the second form.
"""
import collections
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

UNITS = ("tu_dec_128_5", "tu_dec_128_3", "tu_dec_256_5", "tu_dec_256_3", "tu_decoder")
META = (".vgpr_count", ".sgpr_count", ".sgpr_spill_count", ".vgpr_spill_count", ".private_segment_fixed_size", ".group_segment_fixed_size",
        ".amdhsa_next_free_vgpr", ".amdhsa_next_free_sgpr")
GATED = re.compile(r"^(v_|ds_|buffer_|global_|flat_|scratch_|s_barrier|s_waitcnt|s_load_|s_buffer_load_)")


def listing(tree, out, lib, defines, unit, flags, reuse):
    dst = os.path.join(out, lib.replace(".so", ""), unit + ".s")
    os.makedirs(os.path.dirname(dst), exist_ok=True)
    if not (reuse and os.path.exists(dst)):
        src = os.path.join(tree, "efficientspeech_amd", "csrc", unit + ".hip")
        subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + flags + defines + ["--cuda-device-only", "-S", src, "-o", dst])
    return re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid_X", open(dst).read())


def facts(text):
    """per kernel symbol: the metadata fields; for the unit: the mnemonic histogram"""
    meta, hist, name = collections.defaultdict(dict), collections.Counter(), None
    for line in text.splitlines():
        s = line.strip()
        m = re.match(r"\.amdhsa_kernel\s+(\S+)", s)
        if m:
            name = m.group(1)
        m = re.match(r"\.name:\s+(\S+)", s)
        if m:
            name = m.group(1)
        for k in META:
            if s.startswith(k + " ") or s.startswith(k + ":"):
                meta[name][k] = s.split()[-1]
        if line.startswith("\t") and s and s[0] not in ".;" and not s.endswith(":"):
            hist[s.split()[0]] += 1
    return meta, hist


TRAFFIC = re.compile(r"^(buffer_|global_|flat_|scratch_|ds_|v_mfma_|s_barrier)")


def symbols(text):
    """per function symbol (the listing split at its `_Z...:` labels): the body's text, its code size, its memory / matrix / barrier mnemonics"""
    out = {}
    for part in re.split(r"^(?=_Z\w+:)", text, flags=re.M)[1:]:
        if ".Lfunc_end" not in part:
            continue
        body = re.sub(r"BB\d+_", "BB_", part.split(".Lfunc_end")[0])   # (block labels carry the function's ordinal in the unit)
        ops = collections.Counter(s.split()[0] for s in (ln.strip() for ln in body.splitlines()[1:]) if s and s[0] not in ".;" and not s.endswith(":"))
        size = re.search(r"codeLenInByte = (\d+)", part)
        out[part[:part.index(":")]] = (body, int(size.group(1)) if size else -1, {m: n for m, n in ops.items() if TRAFFIC.match(m)})
    return out


def main():
    args = [a for i, a in enumerate(sys.argv[1:], 1) if not a.startswith("--") and sys.argv[i - 1] not in ("--out", "--units")]
    parent, branch = os.path.abspath(args[0]), os.path.abspath(args[1])
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else tempfile.mkdtemp(prefix="dec_isa_")
    units = tuple(sys.argv[sys.argv.index("--units") + 1].split(",")) if "--units" in sys.argv else UNITS
    sys.path.insert(0, branch)
    import __graft_entry__ as ge
    jobs = [(tree, os.path.join(out, tag), lib, d, u, ge.FLAGS, tag == "parent" and "--reuse-parent" in sys.argv)
            for tag, tree in (("parent", parent), ("branch", branch)) for lib, d in ge.VARIANTS.items() for u in units]
    with ThreadPoolExecutor(max_workers=min(len(jobs), 16, os.cpu_count() or 4)) as ex:
        texts = list(ex.map(lambda j: listing(*j), jobs))
    half, bad = len(jobs) // 2, 0
    for (_, _, lib, _, unit, _, _), a, b in zip(jobs[:half], texts[:half], texts[half:]):
        if a == b:
            print(f"{lib:22s} {unit:14s} identical")
            continue
        (ma, ha), (mb, hb) = facts(a), facts(b)
        dm = [(k, f, ma[k].get(f), mb.get(k, {}).get(f)) for k in ma for f in ma[k] if ma[k].get(f) != mb.get(k, {}).get(f)]
        dh = [(m, ha[m], hb[m]) for m in sorted(set(ha) | set(hb)) if ha[m] != hb[m]]
        gated = [d for d in dh if GATED.match(d[0])]
        sa, sb = symbols(a), symbols(b)
        moved = [k for k in sa if k in sb and sa[k][0] != sb[k][0]]
        traffic = [k for k in moved if sa[k][2] != sb[k][2]]
        ok = not dm and not (gated if len(sa) < 2 else traffic) and set(ma) <= set(mb) and set(sa) <= set(sb)
        bad += not ok
        print(f"{lib:22s} {unit:14s} {'second form' if ok else 'DIFFERS'}: metadata {dm or 'equal'}; gated mnemonics {gated or 'equal'}; "
              f"scalar ALU / move {[d for d in dh if not GATED.match(d[0])] or 'equal'}")
        print(f"    {len(sa) - len(moved)} of {len(sa)} symbols identical; missing in the branch: {sorted(set(sa) - set(sb)) or 'none'}")
        for k in moved:   # which kernels' text differs, their code sizes, and whether they issue the same memory / matrix / barrier operations
            print(f"    differs: {k}  {sa[k][1]} -> {sb[k][1]} bytes; memory / mfma / barrier counts {'equal' if k not in traffic else (sa[k][2], sb[k][2])}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
