#!/usr/bin/env python3
"""Compare two gfx950 device assemblies of hconv.hip kernel by kernel:

    tools/asm_compare.py BEFORE.s AFTER.s [--show NAME]

Both files come from the product's flags plus `--cuda-device-only -S` (what tests/test_kernel_resources.py compiles). A refactor of the __forceinline__ helpers is expected to
leave every kernel's instruction stream IDENTICAL (comments, debug directives and the numbering of local labels aside). Where a stream is not identical the tool prints what
must still agree - the resource figures of the kernel's footer (SGPRs, VGPRs, AGPRs, scratch, occupancy, LDS) and the counts of global_load, s_load, LDS, s_barrier and
v_mul / v_mad instructions - and, with --show NAME, a diff of the kernels whose symbol contains NAME.
Exit status 0: same kernel set, every kernel identical or equal in resources and counts; 1 otherwise. A developer's tool: not part of the test suite or the benchmark."""
import difflib
import re
import sys

# footer line "; <key>: <n>" -> the name it is reported under (compilers print the SGPR total under either spelling)
RESOURCES = {"TotalNumSgprs": "SGPRs", "NumSgprs": "SGPRs", "NumVgprs": "VGPRs", "NumAgprs": "AGPRs", "ScratchSize": "Scratch", "Occupancy": "Occupancy", "LDSByteSize": "LDS"}
REQUIRED = sorted(set(RESOURCES.values()))
COUNTED = {"global_load": r"global_load", "s_load": r"s_load", "lds": r"ds_(read|write|load|store)", "s_barrier": r"s_barrier", "v_mul/mad": r"v_(mul|mad)"}
DIRECTIVE = re.compile(r"\.(loc|file|cfi_|ident|p2align|section|type|size|globl|protected|weak|text)\b")
LOCAL_LABEL = re.compile(r"\.L(BB|tmp|func_begin|func_end)\d+(_\d+)?")
FUNCTION_START = re.compile(r"(_Z\w+|hc_k_\w+):")
FOOTER_LINE = re.compile(r";\s*(\w+):\s*(\d+)")


class Kernel:
    def __init__(self):
        self.code, self.resources, self.labels = [], {}, {}

    def add_instruction(self, line):
        line = line.split(" ; ")[0].split("\t;")[0].strip()        # trailing comment (an operand never holds " ; ")
        if not line or line.startswith(";") or DIRECTIVE.match(line):
            return
        line = LOCAL_LABEL.sub(lambda m: self.labels.setdefault(m.group(0), ".L%d" % len(self.labels)), line)
        self.code.append(re.sub(r"\s+", " ", line))

    def counts(self):
        return {name: sum(1 for ln in self.code if re.match(pat, ln)) for name, pat in COUNTED.items()}


def kernels(path):
    """symbol -> Kernel, in one pass: `symbol:` opens the code, `.amdhsa_kernel` / `.Lfunc_end` closes it, `; Kernel info:` opens the footer, `; Occupancy` is its last line read"""
    found, cur, where = {}, None, "outside"
    for raw in open(path):
        start = FUNCTION_START.match(raw)
        if start:
            cur, where = Kernel(), "code"
            found[start.group(1)] = cur
        elif where == "code":
            if raw.lstrip().startswith((".amdhsa_kernel", ".Lfunc_end")):
                where = "after code"
            else:
                cur.add_instruction(raw)
        elif where == "after code" and raw.startswith("; Kernel info:"):
            where = "footer"
        elif where == "footer":
            m = FOOTER_LINE.match(raw)
            if m and m.group(1) in RESOURCES:
                cur.resources[RESOURCES[m.group(1)]] = int(m.group(2))
            if raw.startswith("; Occupancy"):
                where = "outside"
    found = {name: k for name, k in found.items() if k.resources}       # device functions have no kernel footer
    for name, k in found.items():
        missing = [r for r in REQUIRED if r not in k.resources]
        if missing:
            sys.exit("%s: %s: no %s in the kernel's footer - the footer format is not the one this tool reads" % (path, name, ", ".join(missing)))
    return found


def main(argv):
    show = argv[argv.index("--show") + 1] if "--show" in argv else None
    paths = [a for a in argv[1:] if a not in ("--show", show)]
    if len(paths) != 2:
        sys.exit(__doc__)
    before, after = kernels(paths[0]), kernels(paths[1])
    failed = set(before) != set(after)
    if failed:
        print("kernel sets differ: only before", sorted(set(before) - set(after)), "only after", sorted(set(after) - set(before)))
    identical = 0
    for name in sorted(set(before) & set(after)):
        b, a = before[name], after[name]
        if b.code == a.code and b.resources == a.resources:
            identical += 1
            continue
        equal = b.resources == a.resources and b.counts() == a.counts()
        failed |= not equal
        print("%s %s" % ("DIFFERENT SCHEDULE" if equal else "MISMATCH", name))
        for tag, k in (("before", b), ("after ", a)):
            print("    %s %s %s %d lines" % (tag, k.resources, k.counts(), len(k.code)))
        if show and show in name:
            print("\n".join(difflib.unified_diff(b.code, a.code, "before", "after", lineterm="", n=2)))
    print("%d kernels before, %d after, %d identical" % (len(before), len(after), identical))
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
