"""Compare the gfx950 device code of two builds, kernel by kernel: usage  codeobj_diff.py <build/dev of A> <build/dev of B>
For every translation unit of build.SOURCES the embedded code object is extracted (llvm-objdump --offloading) and three things are compared: the set of
kernel symbols, the disassembly text per kernel, and the per-kernel metadata of the notes (registers, scratch, LDS, kernarg size).  Exit status 1 on any
difference.  (Raw code-object bytes differ between checkouts outside the text -- compare this, not file hashes.)"""
import collections, glob, os, re, shutil, subprocess, sys, tempfile
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from yolosharp_amd.build import SOURCES
LLVM = "/opt/rocm/lib/llvm/bin/"
META = (".vgpr_count", ".agpr_count", ".sgpr_count", ".vgpr_spill_count", ".sgpr_spill_count", ".private_segment_fixed_size", ".group_segment_fixed_size", ".kernarg_segment_size", ".max_flat_workgroup_size", ".wavefront_size")


def kernels(obj, tmp):
    """{symbol: (disassembly lines without addresses, metadata dict or None)} of the gfx950 code object embedded in obj"""
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
        return "absent on one side" if a is None or b is None else "METADATA differs"
    blank = lambda l: re.sub(r"\b([vsa])(\d+|\[\d+:\d+\])", r"\1#", l)
    ca, cb = collections.Counter(map(blank, a[0])), collections.Counter(map(blank, b[0]))
    n = sum(((ca - cb) + (cb - ca)).values())
    return "same metadata; %d / %d instructions, %s" % (len(a[0]), len(b[0]), "the same multiset up to register names" if n == 0 else "%d not matched up to register names" % n)


def main(a_dir, b_dir):
    bad = 0
    with tempfile.TemporaryDirectory() as tmp:
        for tu in SOURCES:
            ka, kb = kernels(os.path.join(a_dir, tu + ".o"), tmp), kernels(os.path.join(b_dir, tu + ".o"), tmp)
            diff = sorted(set(ka) ^ set(kb)) + sorted(k for k in set(ka) & set(kb) if ka[k] != kb[k])
            if diff:
                bad += 1
                print("%-22s %d of %d kernels DIFFER:" % (tu, len(diff), len(set(ka) | set(kb))))
                for k in diff:
                    print("    %s  [%s]\n      A: %s\n      B: %s" % (k, how(ka.get(k), kb.get(k)), ka[k][1] if k in ka else "absent", kb[k][1] if k in kb else "absent"))
            else:
                print("%-22s %d kernels identical (%d instructions)" % (tu, sum(1 for v in ka.values() if v[1]), sum(len(v[0]) for v in ka.values())))
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
