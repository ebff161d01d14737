#!/usr/bin/env python3
"""Per-kernel comparison of two device assembly files (hipcc ... --cuda-device-only -S): for a refactor that must not
change device code.  For every .amdhsa_kernel symbol the function body (`<symbol>:` ... `.Lfunc_end<k>:`) and the
descriptor block (`.amdhsa_kernel <symbol>` ... `.end_amdhsa_kernel`) are compared as text.  The only normalisation:
the function's position in the file, <k> of its local labels `.LBB<k>_<n>` / `.Lfunc_end<k>` and of the loop comments that
name them (`Header=BB<k>_<n>`), is replaced by a constant (kernels come out in the order the host code first mentions
them), and with it the padding between such a label and its comment, which depends on the number of digits of <k>.

    python tools/kernel_identity.py before.s after.s > profiles/<name>_kernel_identity.txt

Exit status 1 if a kernel differs or the symbol sets are not equal."""
import hashlib
import re
import sys


def kernels(path):
    text = open(path).read()
    out = {}
    for m in re.finditer(r"^\s*\.amdhsa_kernel (\S+)\n(.*?)^\s*\.end_amdhsa_kernel", text, re.M | re.S):
        sym, desc = m.group(1), m.group(0)
        b = re.search(r"^%s:[^\n]*\n(.*?)^\.Lfunc_end(\d+):" % re.escape(sym), text, re.M | re.S)
        if not b:
            raise SystemExit(f"{path}: no body for {sym}")
        k = b.group(2)
        body = re.sub(r"BB%s_" % k, "BBk_", b.group(1))
        body = re.sub(r"^(\.LBBk_\d+:) +;", r"\1 ;", body, flags=re.M)  # the comment's column padding behind such a label
        fig = {f: re.search(r"\.amdhsa_%s (\S+)" % a, desc) for f, a in (
            ("vgpr", "next_free_vgpr"), ("sgpr", "next_free_sgpr"), ("accum_offset", "accum_offset"),
            ("lds", "group_segment_fixed_size"), ("scratch", "private_segment_fixed_size"))}
        out[sym] = (hashlib.sha256((body + desc).encode()).hexdigest(), len(body.splitlines()),
                    {f: (v.group(1) if v else "-") for f, v in fig.items()})
    return out


def main():
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    bad = 0
    print("# symbol | sha256(body + descriptor) before | after | body lines | vgpr sgpr accum_offset lds scratch(spill bytes) | verdict")
    for sym in sorted(set(a) | set(b)):
        if sym not in a or sym not in b:
            print(f"{sym} | {'only before' if sym in a else 'only after'} | differs")
            bad += 1
            continue
        same = a[sym][0] == b[sym][0]
        bad += not same
        f = b[sym][2]
        print(f"{sym} | {a[sym][0]} | {b[sym][0]} | {b[sym][1]} | {f['vgpr']} {f['sgpr']} {f['accum_offset']} {f['lds']} "
              f"{f['scratch']} | {'same' if same else 'differs'}")
    print(f"# {len(a)} kernels before, {len(b)} after, {bad} differ")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
