"""VGPR / SGPR / scratch / LDS of the kernels in built objects or the linked library: every gfx950 code object is
taken out of the .hip_fatbin section (one per device unit; the library carries them all) and its AMDGPU
metadata printed.
   python tools/kernel_regs.py OBJECT_OR_LIBRARY ... [--] [name-substring ...]   (several objects: one sorted table)
   python tools/kernel_regs.py --text-hash OBJECT_OR_LIBRARY ...     (size and sha256 of each gfx950 .text)
   python tools/kernel_regs.py --kernel-hash OBJECT_OR_LIBRARY ...   (size and sha256 of each kernel's bytes)
Two builds run the same device code when the sorted tables of both modes are equal (profiles/kernels_split.md)."""
import hashlib
import os
import re
import struct
import subprocess
import sys
import tempfile

B = "/opt/rocm/lib/llvm/bin"
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def code_objects(path, tmp):
    """the gfx950 code objects of every offload bundle in the file's .hip_fatbin section"""
    fat = os.path.join(tmp, "fatbin")
    subprocess.run([f"{B}/llvm-objcopy", "--dump-section", f".hip_fatbin={fat}", path, os.path.join(tmp, "junk")], check=True)
    with open(fat, "rb") as f:
        data = f.read()
    starts = [m.start() for m in re.finditer(re.escape(MAGIC), data)]
    if not starts:
        sys.exit(f"{path}: no uncompressed offload bundle in .hip_fatbin (a compressed one, --offload-compress, is not handled)")
    out = []
    for k, s in enumerate(starts):
        piece = os.path.join(tmp, f"bundle{len(os.listdir(tmp))}")
        with open(piece, "wb") as f:
            f.write(data[s:starts[k + 1] if k + 1 < len(starts) else len(data)])
        lst = subprocess.run([f"{B}/clang-offload-bundler", "--list", "--type=o", f"--input={piece}"], capture_output=True, text=True).stdout.split()
        tgt = [t for t in lst if "gfx950" in t]
        if not tgt:
            continue
        co = piece + ".co"
        subprocess.run([f"{B}/clang-offload-bundler", "--unbundle", "--type=o", f"--input={piece}", f"--targets={tgt[0]}", f"--output={co}"], check=True)
        out.append(co)
    if not out:
        sys.exit(f"{path}: no gfx950 code object in its {len(starts)} offload bundle(s)")
    return out


def second_copy(name, seen, co, path):
    """whether this kernel was already met in another code object.  The library's rocprim / hipcub template kernels
    are emitted by every unit that uses them (their first copy is listed); a kernel of the project's own namespace in
    two units is what a split must not introduce"""
    if seen.setdefault(name, co) == co:
        return False
    if name.startswith("_ZN6yafamd"):
        sys.exit(f"kernel {name} is defined twice (second time in {path})")
    return True


def all_code_objects(paths, tmp):
    """(path, code object) of every input, each input unpacked in a directory of its own (by position)"""
    for k, path in enumerate(paths):
        sub = os.path.join(tmp, str(k))
        os.mkdir(sub)
        for co in code_objects(path, sub):
            yield path, co


def text_hash(path):
    """size and sha256 of the gfx950 .text: two builds with the same line run the same device code"""
    with tempfile.TemporaryDirectory() as tmp:
        for k, co in enumerate(code_objects(path, tmp)):
            text = os.path.join(tmp, "text")
            subprocess.run([f"{B}/llvm-objcopy", "-O", "binary", "--only-section=.text", co, text], check=True)
            with open(text, "rb") as f:
                data = f.read()
            print(f"{path}[{k}]: gfx950 .text {len(data)} bytes sha256 {hashlib.sha256(data).hexdigest()}")


def kernel_bytes(co):
    """{kernel name: its bytes in .text} of one code object (ELF64 little endian; kernels are the FUNC symbols
    that have a NAME.kd descriptor)"""
    with open(co, "rb") as f:
        d = f.read()
    shoff, = struct.unpack_from("<Q", d, 0x28)
    shentsize, shnum, shstrndx = struct.unpack_from("<HHH", d, 0x3A)
    sec = [struct.unpack_from("<IIQQQQIIQQ", d, shoff + k * shentsize) for k in range(shnum)]
    cstr = lambda tab, off: d[tab + off:d.index(b"\0", tab + off)].decode()
    names = [cstr(sec[shstrndx][4], s[0]) for s in sec]
    symtab = sec[names.index(".symtab")]
    strtab = sec[symtab[6]][4]
    syms = {}
    for k in range(symtab[5] // 24):
        st_name, st_info, _, st_shndx, st_value, st_size = struct.unpack_from("<IBBHQQ", d, symtab[4] + 24 * k)
        syms[cstr(strtab, st_name)] = (st_info & 15, st_shndx, st_value, st_size)
    out = {}
    for name, (typ, shndx, value, size) in syms.items():
        if typ == 2 and name + ".kd" in syms:
            s = sec[shndx]
            out[name] = d[s[4] + value - s[3]:s[4] + value - s[3] + size]
    return out


def kernel_hash(paths):
    with tempfile.TemporaryDirectory() as tmp:
        rows, seen = {}, {}
        for path, co in all_code_objects(paths, tmp):
            for name, b in kernel_bytes(co).items():
                if not second_copy(name, seen, co, path):
                    rows[name] = f"{name} {len(b)} {hashlib.sha256(b).hexdigest()}"
    for name in sorted(rows):
        print(rows[name])


def regs(paths, pats):
    rows, seen = [], {}
    with tempfile.TemporaryDirectory() as tmp:
        for path, co in all_code_objects(paths, tmp):
            notes = subprocess.run([f"{B}/llvm-readelf", "--notes", co], capture_output=True, text=True).stdout
            for blk in re.split(r"\n  - \.agpr_count:", notes)[1:]:
                blk = ".agpr_count:" + blk
                g = lambda k: (re.search(r"\." + k + r":\s+(\S+)", blk) or [None, "?"])[1]
                name = g("name")
                if second_copy(name, seen, co, path) or (pats and not any(p in name for p in pats)):
                    continue
                rows.append(f"{name[:70]:70s} vgpr {g('vgpr_count'):>4s} agpr {g('agpr_count'):>4s} sgpr {g('sgpr_count'):>4s} "
                            f"scratch {g('private_segment_fixed_size'):>5s} lds {g('group_segment_fixed_size'):>5s} spill {g('vgpr_spill_count')}")
    for r in rows if len(paths) == 1 else sorted(rows):
        print(r)


def main():
    if sys.argv[1] == "--text-hash":
        for path in sys.argv[2:]:
            text_hash(path)
        return
    if sys.argv[1] == "--kernel-hash":
        kernel_hash(sys.argv[2:])
        return
    # the leading arguments that are files are the objects; what follows (after an optional --) are name substrings
    args = sys.argv[1:]
    n = next((k for k, a in enumerate(args) if a == "--" or not os.path.isfile(a)), len(args))
    regs(args[:n], [a for a in args[n:] if a != "--"])


if __name__ == "__main__":
    main()
