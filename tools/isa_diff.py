#!/usr/bin/env python3
"""Compares the gfx950 device code of two builds of liblmi_hip.so kernel by kernel (developer aid; runs without a GPU).

For every kernel symbol: the metadata note (VGPRs, AGPRs, SGPRs, LDS, scratch, kernel-argument bytes) and the disassembled
body (addresses stripped, alignment padding behind the last instruction not counted), compared by NAME -- the instantiation
order may move.  Prints the kernels only one side has, those whose notes differ and those whose bodies differ.

  python3 tools/isa_diff.py parent/liblmi_hip.so learnedmetricindex_amd/liblmi_hip.so     exit code 1 if a shared kernel's body differs"""
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import isa_guard  # noqa: E402

NOTE_KEYS = (".vgpr_count", ".agpr_count", ".sgpr_count", ".private_segment_fixed_size", ".group_segment_fixed_size", ".kernarg_segment_size")


def device_code(so_path):
    """({kernel: note dict}, {kernel: [instruction, ..]}) of the library's gfx950 code object."""
    with tempfile.TemporaryDirectory() as wd:
        co = isa_guard.extract_code_object(so_path, wd)
        notes = isa_guard.kernel_notes(co)
        text = subprocess.check_output([f"{isa_guard.LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", co], text=True)
    bodies, cur = {}, None
    for line in text.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m:
            cur = m.group(1)
            bodies[cur] = []
        elif cur and line.strip():
            bodies[cur].append(re.sub(r"//.*$", "", re.sub(r"^\s*[0-9a-f]+:\s*", "", line)).strip())
    for body in bodies.values():
        # (the code object's last kernel also carries the section's trailing padding, which objdump elides as a line of "...")
        while body and (body[-1].startswith("s_nop") or body[-1].startswith("s_code_end") or body[-1] == "..."):
            body.pop()
    return notes, {k: v for k, v in bodies.items() if k in notes}


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    (na, ba), (nb, bb) = device_code(sys.argv[1]), device_code(sys.argv[2])
    shared = sorted(set(ba) & set(bb))
    print(f"kernels: {len(ba)} / {len(bb)}, shared {len(shared)}")
    for k in sorted(set(ba) - set(bb)):
        print(f"  only in the first:  {k}")
    for k in sorted(set(bb) - set(ba)):
        print(f"  only in the second: {k}  ({len(bb[k])} instructions, "
              + ", ".join(f"{key[1:]} {nb[k].get(key)}" for key in NOTE_KEYS[:5]) + ")")
    n_body = 0
    for k in shared:
        dn = [(key[1:], na[k].get(key), nb[k].get(key)) for key in NOTE_KEYS if na[k].get(key) != nb[k].get(key)]
        if dn:
            print(f"  note differs: {k}: " + ", ".join(f"{key} {a} -> {b}" for key, a, b in dn))
        if ba[k] != bb[k]:
            n_body += 1
            print(f"  BODY differs: {k}: {len(ba[k])} -> {len(bb[k])} instructions")
    print(f"instructions compared: {sum(len(ba[k]) for k in shared)}; shared kernels whose bodies differ: {n_body}")
    sys.exit(1 if n_body else 0)


if __name__ == "__main__":
    main()
