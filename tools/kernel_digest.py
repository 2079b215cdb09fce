#!/usr/bin/env python3
"""Digest of the device code of every kernel in a library (or object file) built by hipcc, no GPU needed:
    python tools/kernel_digest.py ldsr_amd/libldsr_hip.so > a.txt
prints one `digest name` line per device function (names demangled, sorted) and, on stderr, their count and
one combined hash.  Two builds hold the same device code exactly when the outputs are equal: a refactor of
the host side, of the build or of compile-time switches is checked with `diff`.
A digest covers the function's machine code and, for a kernel, its descriptor (register counts, LDS, scratch,
modes) without the descriptor's offset to the code, which depends on where the unit's linker put it.
The code objects are the offload bundles hipcc embeds (`CCOB`: zstd-compressed, see
tests/test_abi_and_host.py test_code_object_is_gfx950_only)."""
import hashlib
import struct
import subprocess
import sys

BUNDLE = b"__CLANG_OFFLOAD_BUNDLE__"


def _unbundle(raw):
    """gfx950 ELF images of an uncompressed offload bundle"""
    (n,) = struct.unpack_from("<Q", raw, len(BUNDLE))
    pos = len(BUNDLE) + 8
    for _ in range(n):
        off, size, idlen = struct.unpack_from("<QQQ", raw, pos)
        ident = raw[pos + 24:pos + 24 + idlen]
        pos += 24 + idlen
        if b"amdgcn" in ident and size:
            yield raw[off:off + size]


def code_objects(path):
    """every device ELF image embedded in the file"""
    import pyarrow as pa
    blob = open(path, "rb").read()
    i = 0
    while True:
        i = blob.find(b"CCOB", i)
        if i < 0:
            break
        total, usize, _ = struct.unpack_from("<QQQ", blob, i + 8)
        yield from _unbundle(pa.Codec("zstd").decompress(blob[i + 32:i + total], usize).to_pybytes())
        i += total


def functions(elf):
    """(mangled name, code bytes, kernel descriptor bytes or b"") of every function of a device ELF image"""
    assert elf[:6] == b"\x7fELF\x02\x01", "not a little-endian ELF64 image"
    shoff, = struct.unpack_from("<Q", elf, 0x28)
    shentsize, shnum, _ = struct.unpack_from("<HHH", elf, 0x3A)
    sections = [struct.unpack_from("<IIQQQQIIQQ", elf, shoff + k * shentsize) for k in range(shnum)]
    symtabs = [s for s in sections if s[1] == 2] or [s for s in sections if s[1] == 11]     # .symtab, else .dynsym
    _, _, _, _, off, size, link, _, _, entsize = symtabs[0]
    stroff = sections[link][4]
    syms = {}
    for o in range(off, off + size, entsize):
        name, info, _, shndx, value, ssize = struct.unpack_from("<IBBHQQ", elf, o)
        if shndx == 0 or shndx >= shnum or (info & 15) not in (1, 2):        # defined objects and functions
            continue
        end = elf.index(b"\0", stroff + name)
        base = sections[shndx]
        syms[elf[stroff + name:end].decode()] = (info & 15, elf[base[4] + value - base[3]:base[4] + value - base[3] + ssize])
    for name, (kind, body) in syms.items():
        if kind != 2:
            continue
        kd = syms.get(name + ".kd", (0, b""))[1]
        if kd:
            assert len(kd) == 64, (name, len(kd))
            kd = kd[:16] + bytes(8) + kd[24:]            # (KERNEL_CODE_ENTRY_BYTE_OFFSET)
        yield name, body, kd


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout
    return out.split("\n")[:len(names)]


def digests(path):
    """{demangled name: digest}; a function emitted into several code objects lists every distinct digest"""
    found = {}
    for elf in code_objects(path):
        for name, body, kd in functions(elf):
            found.setdefault(name, set()).add(hashlib.sha256(body + kd).hexdigest()[:16])
    names = sorted(found)
    return {d: "+".join(sorted(found[m])) for m, d in zip(names, demangle(names))}


if __name__ == "__main__":
    table = digests(sys.argv[1])
    lines = ["%s %s\n" % (table[k], k) for k in sorted(table)]
    sys.stdout.writelines(lines)
    sys.stderr.write("%d device functions, combined %s\n" % (len(lines), hashlib.sha256("".join(lines).encode()).hexdigest()[:16]))
