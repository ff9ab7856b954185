"""Per-kernel comparison of the device code of two built libraries: python scripts/isa_diff.py <old.so> <new.so> [--renames FILE]
(no GPU needed).  For every kernel symbol: the instruction stream (isa_lint.device_disassembly with what depends on the position in
the code object taken off: addresses, encodings and branch-target notes, i.e. the comment column) and the kernel's metadata entry
(register counts, LDS and scratch bytes, kernarg layout, workgroup size) as text.  Kernels are matched by their demangled name without
the parameter list; --renames names a text file whose two-column table rows "| `old` | `new` |" are the old -> new pairs (a
markdown file does: profiles/csrc_prune_isa.md is its own rename table).  Exit status 1 if a common kernel differs or a kernel was added."""
import difflib, os, re, shutil, subprocess, sys, tempfile
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "deeppointmap_amd", "csrc"))
import isa_lint

BIN = os.path.dirname(isa_lint._find_objdump())


def streams(lib):
    """-> {mangled symbol: [instruction lines]} over all code objects of the library"""
    out, cur = {}, None
    for line in isa_lint.device_disassembly(lib):
        m = re.match(r"[0-9a-f]+ <([^>]+)>:$", line)
        if m:
            assert m.group(1) not in out, f"{m.group(1)}: in two code objects"
            cur = out[m.group(1)] = []
        elif cur is not None and line.startswith(("\t", " ")):
            cur.append(line.split("//")[0].strip())
    return out


def metadata(lib):
    """-> {mangled kernel name: its amdhsa.kernels entry without the two lines that carry the name}, {name: code object number}"""
    tmp = tempfile.mkdtemp(prefix="dpm_isa_")
    try:
        shutil.copy(lib, os.path.join(tmp, "lib.so"))
        subprocess.run([os.path.join(BIN, "llvm-objdump"), "--offloading", "lib.so"], cwd=tmp, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        meta, where = {}, {}
        for f in sorted((f for f in os.listdir(tmp) if "hipv4-amdgcn" in f), key=lambda f: int(f.split(".")[2])):
            notes = subprocess.run([os.path.join(BIN, "llvm-readelf"), "--notes", os.path.join(tmp, f)], check=True, capture_output=True, text=True).stdout
            kernels = notes.split("amdhsa.kernels:")[1].split("\namdhsa.")[0] if "amdhsa.kernels:" in notes else ""
            for entry in re.split(r"\n  - ", kernels)[1:]:
                name = re.search(r"\.name:\s+(\S+)", entry).group(1)
                meta[name] = [l.rstrip() for l in entry.splitlines() if not re.match(r"\s*\.(name|symbol):", l)]
                where[name] = int(f.split(".")[2])
        return meta, where
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def short_names(symbols):
    """mangled -> demangled without `(anonymous namespace)::` and the parameter list"""
    syms = sorted(symbols)
    filt = next((c for c in (os.path.join(BIN, "llvm-cxxfilt"), shutil.which("llvm-cxxfilt"), shutil.which("c++filt")) if c and os.path.exists(c)), None)
    if filt is None:   # no demangler: the mangled names (a rename table then has to hold those)
        return {s: s for s in syms}
    dem = subprocess.run([filt], input="\n".join(syms), check=True, capture_output=True, text=True).stdout.splitlines()
    res = {}
    for s, d in zip(syms, dem):
        d = d.replace("(anonymous namespace)::", "")
        d = re.sub(r"^void ", "", d)
        depth = 0
        for i, c in enumerate(d):   # cut at the first '(' outside template brackets
            depth += c == "<"
            depth -= c == ">"
            if c == "(" and depth == 0:
                d = d[:i]
                break
        res[s] = d
    assert len(set(res.values())) == len(res), "two symbols with one short name"
    return res


def load(lib):
    code, (meta, where) = streams(lib), metadata(lib)
    names = short_names(code)
    return {names[s]: (code[s], meta.get(s), where.get(s)) for s in code}


def main(argv):
    renames = {}
    if "--renames" in argv:
        i = argv.index("--renames")
        for line in open(argv[i + 1]):
            m = re.fullmatch(r"\|\s*`([^`]+)`\s*\|\s*`([^`]+)`\s*\|\s*", line)
            if m:
                renames[m.group(1)] = m.group(2)
        argv = argv[:i] + argv[i + 2:]
    old, new = load(argv[1]), load(argv[2])
    for o, n in renames.items():
        assert o in old and n in new and o not in new, f"rename {o} -> {n}: not such a pair in these libraries"
        old[n] = old.pop(o)
    removed, added, common = sorted(set(old) - set(new)), sorted(set(new) - set(old)), sorted(set(old) & set(new))
    differ = []
    for k in common:
        (c0, m0, _), (c1, m1, _) = old[k], new[k]
        if c0 != c1 or m0 != m1:
            differ.append(k)
            print(f"DIFFERS: {k}")
            for d in list(difflib.unified_diff(m0 or [], m1 or [], "old metadata", "new metadata", lineterm="", n=0))[:40]:
                print("    " + d)
            for d in list(difflib.unified_diff(c0, c1, "old code", "new code", lineterm="", n=1))[:80]:
                print("    " + d)
    objs = sorted({w for _, _, w in new.values() if w is not None} | {w for _, _, w in old.values() if w is not None})
    print("code object (in link order; named by its first kernel): kernels old -> new")
    for w in objs:
        a, b = [sum(1 for v in lib.values() if v[2] == w) for lib in (old, new)]
        print(f"  {w:2d} {next((k.split('<')[0] for k, v in sorted(new.items()) if v[2] == w), ''):34s} {a:3d} -> {b:3d}")
    print(f"symbols: {len(old)} -> {len(new)}; renamed {len(renames)}; removed {len(removed)}; added {len(added)}; "
          f"common {len(common)}, of them identical {len(common) - len(differ)}, different {len(differ)}")
    for k in removed:
        print(f"  removed: {k}")
    for k in added:
        print(f"  ADDED: {k}")
    return 1 if differ or added else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
