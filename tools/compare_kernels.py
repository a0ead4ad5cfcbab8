"""Are the device kernels of two builds the same?  For a host-only change: compares, kernel by kernel, the gfx950 code of every
object file of two build directories (acoustic_locating_vq-vae_amd/build or build_dbg of two checkouts).

    python tools/compare_kernels.py OLD_BUILD_DIR NEW_BUILD_DIR [more OLD NEW pairs]

Per object: the .hip_fatbin section is dumped, its gfx950 code object unbundled, and three things are compared keyed by kernel
symbol -- the set of kernels, each kernel's disassembly (addresses and address comments stripped) and each kernel's metadata
entry (registers, LDS, scratch, kernarg layout).  Whole files or whole .text sections are NOT compared: they differ between
two builds of the same source (the per-build unit id) and whenever the host code names the kernels in another order.  The
literal of the s_add_u32 behind an s_getpc_b64 (the distance from there to a __device__ variable) is blanked: it moves with the
size of every kernel that lies between, so an untouched kernel of an object whose other kernels changed would differ by it alone.
Code and metadata are reported separately ("code of", "metadata of", "code and metadata of"), the changed metadata lines with
their values.  Prints one line per object and a total; exit status 1 if anything differs.

    python tools/compare_kernels.py --stats BUILD_DIR REGEX

lists instead the kernels of one build whose symbol matches REGEX: instructions, registers, spilled VGPRs, scratch, static LDS."""
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/lib/llvm/bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"


def _run(*cmd):
    return subprocess.run(cmd, check=True, capture_output=True, text=True).stdout


def code_object(obj, tmp):
    fat, co = os.path.join(tmp, "fatbin"), os.path.join(tmp, "co")
    for f in (fat, co):
        if os.path.exists(f):
            os.remove(f)
    try:
        _run(os.path.join(LLVM, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, obj)
    except subprocess.CalledProcessError:
        return None                                           # an object without device code (no such section)
    _run(os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--targets=" + TARGET, "--input=" + fat, "--output=" + co)
    return co


def kernels(co):
    """{kernel symbol: (disassembly, metadata entry)} of one code object."""
    notes = _run(os.path.join(LLVM, "llvm-readelf"), "--notes", co)
    by_name, entry = {}, None
    for line in notes.split("amdhsa.kernels:", 1)[-1].splitlines()[1:] + ["end"]:
        if not line.startswith("    ") and entry:        # "  - " opens the next entry, anything less indented ends the list
            name = [ln.split()[-1] for ln in entry if ln.startswith("    .name:") or ln.startswith("  - .name:")]
            by_name[name[0]] = "\n".join(entry)
            entry = None
        if line and not line.startswith(" "):                 # amdhsa.target: -- the kernel list is over
            break
        if line.startswith("  - "):
            entry = []
        if entry is not None and line.strip():
            entry.append(line.rstrip())
    dis = _run(os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", "--no-leading-addr", co)
    code, sym = {}, None
    for line in dis.splitlines():
        m = re.match(r"^(?:[0-9a-f]+ )?<(\S+)>:$", line)
        if m:
            sym = m.group(1)
            code[sym] = []
        elif sym is not None and line.strip() and line.strip() != "...":   # "...": zero padding after the section's last kernel
            ins = re.sub(r"\s*//.*$", "", line).strip()
            if code[sym] and code[sym][-1].startswith("s_getpc_b64") and ins.startswith("s_add_u32"):
                ins = re.sub(r"0x[0-9a-f]+$", "<pc-relative>", ins)
            code[sym].append(ins)
    return {k: ("\n".join(code.get(k, ["<no code>"])), by_name[k]) for k in by_name}


def compare(old_dir, new_dir, tmp):
    objs_old = {f for f in os.listdir(old_dir) if f.endswith(".o")}
    objs_new = {f for f in os.listdir(new_dir) if f.endswith(".o")}
    nobj = nker = ndiff = 0
    for f in sorted(objs_old ^ objs_new):
        print("DIFF object only on one side: %s" % f)
        ndiff += 1
    for f in sorted(objs_old & objs_new):
        sides = []
        for d in (old_dir, new_dir):
            co = code_object(os.path.join(d, f), tmp)
            sides.append(kernels(co) if co else {})
        a, b = sides
        bad = sorted(set(a) ^ set(b))
        for k in bad:
            print("DIFF %s: kernel on one side only: %s" % (f, k))
        for k in sorted(set(a) & set(b)):
            what = [w for i, w in enumerate(("code", "metadata")) if a[k][i] != b[k][i]]   # reported separately: a kernel whose
            if what:                                          # code moved may still have to keep its registers, LDS and scratch
                bad.append(k)
                print("DIFF %s: %s of %s" % (f, " and ".join(what), k))
            if "metadata" in what:
                for la, lb in zip(a[k][1].splitlines(), b[k][1].splitlines()):
                    if la != lb:
                        print("       %s  ->  %s" % (la.strip(), lb.strip()))
        print("%-28s %3d kernels, %d differences" % (f, len(set(a) | set(b)), len(bad)))
        nobj, nker, ndiff = nobj + 1, nker + len(set(a) | set(b)), ndiff + len(bad)
    return nobj, nker, ndiff


def stats(build_dir, pattern, tmp):
    """One line per kernel of build_dir whose (mangled) symbol matches the regular expression: instructions, registers, spilled
    VGPRs, scratch and static LDS bytes, from the disassembly and the metadata entry."""
    keys = (".vgpr_count", ".agpr_count", ".sgpr_count", ".vgpr_spill_count", ".private_segment_fixed_size", ".group_segment_fixed_size")
    print("%-72s %6s %5s %5s %5s %7s %8s %6s" % ("kernel", "instr", "vgpr", "agpr", "sgpr", "spilled", "scratch", "lds"))
    for f in sorted(f for f in os.listdir(build_dir) if f.endswith(".o")):
        co = code_object(os.path.join(build_dir, f), tmp)
        for k, (code, meta) in sorted((kernels(co) if co else {}).items()):
            if re.search(pattern, k):
                val = {ln.split(":")[0].strip(" -"): ln.split(":")[1].strip() for ln in meta.splitlines() if ":" in ln}
                print("%-72s %6d " % (k, len([ln for ln in code.splitlines() if not ln.endswith(":")])) +
                      "%5s %5s %5s %7s %8s %6s" % tuple(val.get(key, "-") for key in keys))


def main(argv):
    if len(argv) == 3 and argv[0] == "--stats":               # python tools/compare_kernels.py --stats BUILD_DIR REGEX
        with tempfile.TemporaryDirectory() as tmp:
            stats(argv[1], argv[2], tmp)
        return 0
    if len(argv) < 2 or len(argv) % 2:
        sys.exit(__doc__)
    tot = [0, 0, 0]
    with tempfile.TemporaryDirectory() as tmp:
        for i in range(0, len(argv), 2):
            print("== %s  vs  %s" % (argv[i], argv[i + 1]))
            for j, v in enumerate(compare(argv[i], argv[i + 1], tmp)):
                tot[j] += v
    print("objects compared: %d, kernels compared: %d, differences: %d" % tuple(tot))
    return 1 if tot[2] else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
