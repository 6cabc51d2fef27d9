"""Compare the gfx950 device code of two builds, kernel by kernel: usage  codeobj_diff.py <build/dev of A> <build/dev of B>
For every translation unit of build.SOURCES (of either checkout: a .o that exists on one side only counts as empty) the embedded code object is extracted
(llvm-objdump --offloading) and three things are compared: the set of kernel symbols, the disassembly text per kernel, and the per-kernel metadata of the notes
(registers, scratch, LDS, kernarg size).  Kernels are pooled by symbol over all translation units of a side, so one that moved to another file is compared with
itself; the report is per kernel under the unit(s) that hold it, and a unit whose kernels are all unchanged is "identical".  Exit status 1 on any difference.
(Raw code-object bytes differ between checkouts outside the text -- compare this, not file hashes.)"""
import collections, glob, os, re, shutil, subprocess, sys, tempfile
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from yolosharp_amd.build import SOURCES
LLVM = "/opt/rocm/lib/llvm/bin/"
META = (".vgpr_count", ".agpr_count", ".sgpr_count", ".vgpr_spill_count", ".sgpr_spill_count", ".private_segment_fixed_size", ".group_segment_fixed_size", ".kernarg_segment_size", ".max_flat_workgroup_size", ".wavefront_size")


def kernels(obj, tmp):
    """{symbol: (disassembly lines without addresses, metadata dict or None)} of the gfx950 code object embedded in obj"""
    if not os.path.exists(obj):                            # a translation unit the other side has and this one does not
        return {}
    local = os.path.join(tmp, os.path.basename(obj))
    shutil.copy(obj, local)
    subprocess.run([LLVM + "llvm-objdump", "--offloading", local], check=True, cwd=tmp, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    co = [f for f in glob.glob(local + "*gfx950*") if f != local]
    if not co:                                             # a translation unit without device code
        return {}
    assert len(co) == 1, (obj, co)
    dis = subprocess.run([LLVM + "llvm-objdump", "-d", "--no-show-raw-insn", "--no-leading-addr", co[0]], check=True, stdout=subprocess.PIPE, text=True).stdout
    text, cur = {}, None
    for line in dis.splitlines():
        m = re.match(r"^[0-9a-f]* ?<(.+)>:$", line)
        if m:
            cur = text.setdefault(m.group(1), [])
        elif cur is not None and line.strip():
            cur.append(re.sub(r"\s*//.*$", "", line).strip())     # the trailing comment is the instruction's address / encoding
    for lines in text.values():                            # alignment padding up to the next symbol is not part of the kernel
        while lines and lines[-1] in ("s_nop 0", "..."):
            lines.pop()
    notes = subprocess.run([LLVM + "llvm-readelf", "--notes", co[0]], check=True, stdout=subprocess.PIPE, text=True).stdout
    meta = {}
    for block in re.split(r"\n\s*- \.agpr_count:", "\n" + notes)[1:]:
        block = "  .agpr_count:" + block
        name = re.search(r"^\s*\.name:\s*(\S+)", block, re.M).group(1)
        meta[name] = {k: (re.search(r"^\s*" + re.escape(k) + r":\s*(\S+)", block, re.M) or [None, None])[1] for k in META}
    for f in glob.glob(local + "*"):
        os.remove(f)
    assert set(meta) <= set(text), (obj, sorted(set(meta) - set(text)))
    return {k: (text[k], meta.get(k)) for k in text}       # (symbols without metadata are device functions the compiler did not inline)


def how(a, b):
    """what kind of difference: register allocation / instruction order only, or other instructions"""
    if a is None or b is None or a[1] != b[1]:
        if a is None or b is None:
            return "absent on one side"
        keys = [k for k in META if (a[1] or {}).get(k) != (b[1] or {}).get(k)]
        return "METADATA differs: " + ", ".join(keys) + ("; %d / %d instructions" % (len(a[0]), len(b[0])) if keys == [".sgpr_count"] else "")
    blank = lambda l: re.sub(r"\b([vsa])(\d+|\[\d+:\d+\])", r"\1#", l)
    ca, cb = collections.Counter(map(blank, a[0])), collections.Counter(map(blank, b[0]))
    n = sum(((ca - cb) + (cb - ca)).values())
    return "same metadata; %d / %d instructions, %s" % (len(a[0]), len(b[0]), "the same multiset up to register names" if n == 0 else "%d not matched up to register names" % n)


def pool(d, tus, tmp):
    """{symbol: [(translation unit, (text, metadata)), ...]} over all translation units of one side"""
    out = collections.defaultdict(list)
    for tu in tus:
        for k, v in kernels(os.path.join(d, tu + ".o"), tmp).items():
            out[k].append((tu, v))
    return out


def main(a_dir, b_dir):
    tus = list(SOURCES) + sorted({os.path.basename(f)[:-2] for d in (a_dir, b_dir) for f in glob.glob(os.path.join(d, "*.o"))} - set(SOURCES))
    bad = 0
    with tempfile.TemporaryDirectory() as tmp:
        pa, pb = pool(a_dir, tus, tmp), pool(b_dir, tus, tmp)
        body = lambda p, k: sorted((v for _, v in p.get(k, [])), key=repr)   # (a symbol defined in several units: compared as a multiset)
        differ = {k for k in set(pa) | set(pb) if body(pa, k) != body(pb, k)}
        for tu in tus:
            mine = sorted(k for k in set(pa) | set(pb) if any(t == tu for p in (pa, pb) for t, _ in p.get(k, [])))
            diff = [k for k in mine if k in differ]
            if diff:
                bad += 1
                print("%-22s %d of %d kernels DIFFER:" % (tu, len(diff), len(mine)))
                for k in diff:
                    a, b = (p[k][0][1] if k in p else None for p in (pa, pb))
                    where = " / ".join("+".join(t for t, _ in p.get(k, [])) or "-" for p in (pa, pb))
                    print("    %s  (%s)  [%s]\n      A: %s\n      B: %s" % (k, where, how(a, b), a[1] if a else "absent", b[1] if b else "absent"))
            else:
                held = [pa[k][0][1] for k in mine]
                print("%-22s %d kernels identical (%d instructions)" % (tu, sum(1 for v in held if v[1]), sum(len(v[0]) for v in held)))
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
