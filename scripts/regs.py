#!/usr/bin/env python3
"""usage: scripts/regs.py lib.so [name filter]: VGPRs / SGPRs / spills / LDS / private segment of the gfx950 kernels in a built library
(reads the offload bundle inside the .so and the code object's metadata notes; compiles nothing)"""
import re, struct, subprocess, sys, tempfile


def kernel_stats(lib_path, pattern="."):
    """the metadata records (field -> text, as llvm-readelf prints them) of the gfx950 kernels in lib_path whose name matches pattern"""
    data = open(lib_path, "rb").read()
    pat = re.compile(pattern)
    at = data.find(b"__CLANG_OFFLOAD_BUNDLE__")
    assert at >= 0, "no uncompressed offload bundle in " + lib_path
    n, = struct.unpack_from("<Q", data, at + 24)
    p, recs = at + 32, []
    for _ in range(n):
        off, size, tl = struct.unpack_from("<QQQ", data, p); p += 24
        triple = data[p:p + tl].decode(); p += tl
        if "gfx950" not in triple:
            continue
        with tempfile.NamedTemporaryFile(suffix=".co") as f:
            f.write(data[at + off:at + off + size]); f.flush()
            notes = subprocess.run(["/opt/rocm/lib/llvm/bin/llvm-readelf", "--notes", f.name], capture_output=True, text=True).stdout
        cur = {}
        for line in notes.splitlines():
            m = re.match(r"\s+-?\s*\.(\w+):\s+(\S+)", line)
            if not m:
                continue
            k, v = m.groups()
            if k == "group_segment_fixed_size" and "name" in cur:   # a new kernel record starts (fields come sorted by key)
                cur = {}
            cur[k] = v
            if k == "vgpr_spill_count" and pat.search(cur.get("name", "")):
                recs.append(dict(cur))
    return recs


def occupancy_line(r):
    """a record as the *_times.py scripts write it to profiles/*/kernel_stats.txt: with the waves per SIMD the 512-register file admits"""
    vg = int(r["vgpr_count"])
    occ = min(8, 512 // max(8, (vg + 7) // 8 * 8))
    return (f"{r['name']:60s} vgpr {vg:4d} spill {r['vgpr_spill_count']:>3s} sgpr {r.get('sgpr_count'):>3s} sgpr_spill "
            f"{r.get('sgpr_spill_count'):>3s} lds {r.get('group_segment_fixed_size')} private "
            f"{r.get('private_segment_fixed_size')} occupancy {occ} waves/SIMD")


if __name__ == "__main__":
    for r in kernel_stats(sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else "."):
        print(f"{r.get('name'):70s} vgpr {r.get('vgpr_count'):>4s} spill {r['vgpr_spill_count']:>3s} sgpr {r.get('sgpr_count'):>3s} "
              f"sgpr_spill {r.get('sgpr_spill_count'):>3s} lds {r.get('group_segment_fixed_size')} "
              f"private {r.get('private_segment_fixed_size')}")
