#!/usr/bin/env python3
"""Are the kernels of two source trees the same machine code?

    python tools/kernel_identity.py OLD_TREE NEW_TREE --old kron_v5.hip \
        --new kron_v5_p1.hip kron_v5_p2.hip ... [--both kron_dpp.hip ...] [--out report.md]

Compiles the device side of each listed ``poms_amd/csrc`` file of each tree with the flags
of ``poms_amd/build.py`` (that tree's own copy) into a gfx950 code object, and compares the
kernels by symbol name over the union of each side's files:

  * the function's bytes in ``.text`` (branches are pc-relative, so a kernel's bytes do
    not depend on where the linker put it);
  * its resource figures from the code object's metadata note (VGPRs, AGPRs, SGPRs, LDS
    and scratch bytes, wavefront size, kernarg size) and its 64-byte kernel descriptor,
    the descriptor's own offset to the code excepted.

One thing in a kernel's bytes does depend on the layout: the 32-bit literal of a
pc-relative address of a ``__device__`` variable (``s_getpc_b64`` followed by
``s_add_u32`` / ``s_addc_u32`` with a literal).  Kernels that differ only in such literals
are counted as identical and listed as "masked"; nothing else is masked.

The tool only diffs.  It reports kernels found in one tree only and kernels that differ,
and exits 1 if a kernel differs or exists only in the new tree.  It compiles for minutes
(``--jobs``); the time of every compile is part of the report.  Not a test.
"""
from __future__ import annotations

import argparse
import concurrent.futures as cf
import hashlib
import importlib.util
import re
import struct
import subprocess
import sys
import tempfile
import time
from pathlib import Path


def _build_mod(tree: Path):
    spec = importlib.util.spec_from_file_location(f"_build_{abs(hash(str(tree)))}", tree / "poms_amd" / "build.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _tool(hipcc: str, name: str) -> str:
    for cand in (Path(hipcc).resolve().parent.parent / "llvm" / "bin" / name,
                 Path(hipcc).resolve().parent.parent / "lib" / "llvm" / "bin" / name):
        if cand.exists():
            return str(cand)
    raise RuntimeError(f"{name} not found beside {hipcc}")


def compile_device(tree: Path, name: str, out: Path, reuse: bool = False) -> float:
    """The device code object of csrc/<name>, with build.py's flags; returns the seconds
    (kept beside the code object, so that ``reuse`` can report them again)."""
    secs = out.with_suffix(".secs")
    if reuse and out.exists() and secs.exists():
        return float(secs.read_text())
    b = _build_mod(tree)
    cmd = [b._hipcc(), *b._flags(), "-I", str(tree / "include"), "--cuda-device-only",
           "--no-gpu-bundle-output", "-c", str(tree / "poms_amd" / "csrc" / name), "-o", str(out)]
    t0 = time.time()
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"hipcc failed on {tree}/{name}:\n{r.stdout}\n{r.stderr}")
    secs.write_text(f"{time.time() - t0:.1f}")
    return float(secs.read_text())


def _sections(data: bytes):
    shoff, = struct.unpack_from("<Q", data, 0x28)
    shentsize, shnum, shstrndx = struct.unpack_from("<HHH", data, 0x3A)
    raw = [struct.unpack_from("<IIQQQQIIQQ", data, shoff + i * shentsize) for i in range(shnum)]
    stroff = raw[shstrndx][4]
    secs = []
    for (nm, typ, _fl, addr, off, size, link, _info, _al, entsize) in raw:
        end = data.index(b"\0", stroff + nm)
        secs.append(dict(name=data[stroff + nm:end].decode(), type=typ, addr=addr, off=off, size=size, link=link,
                         entsize=entsize))
    return secs


def _mask_pcrel(code: bytes) -> tuple[bytes, int]:
    """Zero the literal of s_add_u32 / s_addc_u32 within 6 dwords after an s_getpc_b64."""
    n = len(code) // 4
    w = list(struct.unpack_from(f"<{n}I", code))
    masked = 0
    for i in range(n):
        if (w[i] & 0xFF80FFFF) != 0xBE801C00:   # SOP1 s_getpc_b64 (gfx9)
            continue
        j = i + 1
        while j < min(i + 7, n - 1):
            op = (w[j] >> 23) & 0x1FF
            if op in (0x100, 0x104) and ((w[j] & 0xFF) == 0xFF or ((w[j] >> 8) & 0xFF) == 0xFF):
                w[j + 1] = 0   # SOP2 s_add_u32 (0) / s_addc_u32 (4) with a 32-bit literal
                masked += 1
                j += 2
            else:
                j += 1
    return struct.pack(f"<{n}I", *w), masked


def kernels_of(co: Path, readelf: str) -> dict[str, dict]:
    data = co.read_bytes()
    secs = _sections(data)
    symtab = next(s for s in secs if s["name"] == ".symtab")
    strtab = secs[symtab["link"]]
    syms = {}
    for i in range(symtab["size"] // 24):
        nm, info, _other, shndx, value, size = struct.unpack_from("<IBBHQQ", data, symtab["off"] + 24 * i)
        end = data.index(b"\0", strtab["off"] + nm)
        syms[data[strtab["off"] + nm:end].decode()] = (info & 15, shndx, value, size)
    # resource figures: the metadata note, as llvm-readelf prints it
    notes = subprocess.run([readelf, "--notes", str(co)], capture_output=True, text=True, check=True).stdout
    meta = {}
    keys = (".agpr_count", ".group_segment_fixed_size", ".kernarg_segment_size", ".private_segment_fixed_size",
            ".sgpr_count", ".sgpr_spill_count", ".vgpr_count", ".vgpr_spill_count", ".wavefront_size",
            ".max_flat_workgroup_size", ".uses_dynamic_stack")
    for block in re.split(r"\n\s*- \.agpr_count:", "\n" + notes)[1:]:
        block = ".agpr_count:" + block
        vals = {k: m.group(1) for k in keys if (m := re.search(rf"(?m)^\s*{re.escape(k)}:\s*(\S+)", block))}
        m = re.search(r"(?m)^\s*\.name:\s*(\S+)", block)
        if m:
            meta[m.group(1)] = vals
    out = {}
    for name, (typ, shndx, value, size) in syms.items():
        if typ != 2 or name + ".kd" not in syms:   # STT_FUNC with a kernel descriptor
            continue
        sec = secs[shndx]
        code = data[sec["off"] + value - sec["addr"]:][:size]
        _t, kshndx, kvalue, ksize = syms[name + ".kd"]
        ksec = secs[kshndx]
        kd = bytearray(data[ksec["off"] + kvalue - ksec["addr"]:][:ksize])
        kd[16:24] = b"\0" * 8   # kernel_code_entry_byte_offset: where the linker put the code
        if name not in meta:
            raise RuntimeError(f"{co}: no metadata for {name}")
        out[name] = dict(code=code, kd=bytes(kd), meta=meta[name])
    return out


def collect(tree: Path, files: list[str], work: Path, jobs: int, readelf: str, reuse: bool = False):
    tag = hashlib.sha1(str(tree.resolve()).encode()).hexdigest()[:8]
    with cf.ThreadPoolExecutor(max_workers=jobs) as ex:
        secs = list(ex.map(lambda f: compile_device(tree, f, work / f"{tag}_{f}.co", reuse), files))
    kernels, per_file = {}, []
    for f, s in zip(files, secs):
        k = kernels_of(work / f"{tag}_{f}.co", readelf)
        dup = set(k) & set(kernels)
        if dup:
            raise RuntimeError(f"{tree}: {f} repeats kernels of another file, e.g. {sorted(dup)[0]}")
        kernels.update(k)
        per_file.append((f, s, len(k)))
    return kernels, per_file


def demangle(names: list[str], hipcc: str) -> list[str]:
    try:
        r = subprocess.run([_tool(hipcc, "llvm-cxxfilt")], input="\n".join(names), capture_output=True, text=True)
        if r.returncode == 0:
            return [re.sub(r"\(.*", "", n) for n in r.stdout.splitlines()]
    except RuntimeError:
        pass
    return names


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("old_tree", type=Path)
    ap.add_argument("new_tree", type=Path)
    ap.add_argument("--old", nargs="*", default=[], help="csrc files of the old tree only")
    ap.add_argument("--new", nargs="*", default=[], help="csrc files of the new tree only")
    ap.add_argument("--both", nargs="*", default=[], help="csrc files of both trees")
    ap.add_argument("--jobs", type=int, default=4)
    ap.add_argument("--work", type=Path, default=None, help="directory for the code objects (default: temporary)")
    ap.add_argument("--reuse-old", action="store_true", help="keep the old tree's code objects found in --work")
    ap.add_argument("--out", type=Path, default=None, help="write the report here as well")
    a = ap.parse_args()
    hipcc = _build_mod(a.new_tree)._hipcc()
    readelf = _tool(hipcc, "llvm-readelf")
    tmp = None
    if a.work is None:
        tmp = tempfile.TemporaryDirectory()
        a.work = Path(tmp.name)
    a.work.mkdir(parents=True, exist_ok=True)
    old, old_files = collect(a.old_tree, a.old + a.both, a.work, a.jobs, readelf, a.reuse_old)
    new, new_files = collect(a.new_tree, a.new + a.both, a.work, a.jobs, readelf)

    only_old = sorted(set(old) - set(new))
    only_new = sorted(set(new) - set(old))
    differ, masked = [], []
    for name in sorted(set(old) & set(new)):
        o, n = old[name], new[name]
        what = [k for k in ("meta", "kd") if o[k] != n[k]]
        if o["code"] != n["code"]:
            (oc, om), (nc, nm) = _mask_pcrel(o["code"]), _mask_pcrel(n["code"])
            if oc == nc and om == nm and om > 0:
                masked.append((name, om))
            else:
                what.append(f"code ({len(o['code'])} -> {len(n['code'])} bytes)")
        if what:
            differ.append((name, ", ".join(what)))

    lines = ["# Kernel identity", "",
             "Device code of the old tree against the new one, per kernel symbol: the function's bytes,",
             "the metadata's resource figures and the kernel descriptor.  Compile times are one",
             f"hipcc process each, {a.jobs} at a time.", "",
             "| tree | file | device compile (s) | kernels |", "|---|---|---|---|"]
    for tree, files in (("old", old_files), ("new", new_files)):
        lines += [f"| {tree} | `{f}` | {s:.0f} | {k} |" for f, s, k in files]
    lines += ["", f"- kernels in the old tree: {len(old)}", f"- kernels in the new tree: {len(new)}",
              f"- in both, identical: {len(set(old) & set(new)) - len(differ)}"
              f" (of these, {len(masked)} after masking pc-relative literals)",
              f"- in both, different: {len(differ)}", f"- only in the old tree: {len(only_old)}",
              f"- only in the new tree: {len(only_new)}", ""]
    for title, names, extra in (("Different", [d[0] for d in differ], [d[1] for d in differ]),
                                ("Only in the new tree", only_new, None),
                                ("Identical after masking the literal of a pc-relative address",
                                 [m[0] for m in masked], [f"{m[1]} literal(s)" for m in masked]),
                                ("Only in the old tree", only_old, None)):
        lines += [f"## {title} ({len(names)})", ""]
        for i, d in enumerate(demangle(names, hipcc)):
            lines.append(f"- `{d}`" + (f": {extra[i]}" if extra else ""))
        lines.append("")
    report = "\n".join(lines)
    print(report)
    if a.out:
        a.out.parent.mkdir(parents=True, exist_ok=True)
        a.out.write_text(report)
    if tmp:
        tmp.cleanup()
    return 1 if differ or only_new else 0


if __name__ == "__main__":
    sys.exit(main())
