"""Compares the kernels of two device-assembly files (make build/kernels.s build/image.s), the method of DESIGN sections 26 and 27:

    python tools/compare_kernel_asm.py <parent.s> <this.s>

A kernel body is the text between its `_Z...:` label and its `.Lfunc_end` label.  Of every line the part from the first `;` on is
dropped; empty lines and assembler directives (lines that start with `.`) are dropped, except `.LBB` block labels, which are
kept and renumbered per function in order of appearance, in label lines and in branch operands alike.  Two bodies are the same
when the remaining lines are equal.  An "instruction line" in the counts printed is a remaining line that is no label."""
import re, sys


def bodies(path):
    text = open(path).read()
    out = {}
    for m in re.finditer(r"\n(_Z\S+):\s*(?:;.*)?\n", text):
        name = m.group(1)
        end = text.find(".Lfunc_end", m.end())
        if end < 0:
            continue
        lines = []
        labels = {}
        for l in text[m.end():end].splitlines():
            l = l.split(";")[0].strip()
            if not l or l.startswith("."):
                if l.endswith(":") and l.startswith(".LBB"):
                    labels[l[:-1]] = "L%d" % len(labels)
                    lines.append(l)
                continue
            lines.append(l)
        def ren(l):
            return re.sub(r"\.LBB\d+_\d+", lambda k: labels.get(k.group(0), k.group(0)), l)
        out[name] = [ren(l) for l in lines]
    return out


a, b = bodies(sys.argv[1]), bodies(sys.argv[2])
same = diff = 0
n_lines = 0
for name, body in a.items():
    if name not in b:
        print("MISSING", name)
        diff += 1
    elif b[name] != body:
        print("DIFFERS", name, len(body), len(b[name]))
        diff += 1
    else:
        same += 1
        n_lines += sum(1 for l in body if not l.endswith(":"))
print("parent kernels %d, identical %d (%d instruction lines), different %d; new file has %d" % (len(a), same, n_lines, diff, len(b)))
for name in b:
    if name not in a:
        print("NEW", name, sum(1 for l in b[name] if not l.endswith(":")))
