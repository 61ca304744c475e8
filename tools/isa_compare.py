"""Compare the gfx950 instruction streams of every kernel in two builds of the library's objects.

usage: python tools/isa_compare.py <before_dir> <after_dir> [out.txt]

Each *.o is unbundled as tools/kernel_regs.sh does and disassembled with llvm-objdump -d --no-show-raw-insn
--no-leading-addr; address comments are stripped and streams are compared per kernel symbol.  Prints one line per kernel
(VGPR / AGPR / SGPR / scratch / LDS and instruction count before and after, identical or not) and a summary."""
import glob
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin")


def _device_object(obj, tmp):
    fat, dev = os.path.join(tmp, "fat.bin"), os.path.join(tmp, os.path.basename(obj) + ".dev")
    r = subprocess.run([f"{LLVM}/llvm-objcopy", f"--dump-section=.hip_fatbin={fat}", obj, os.path.join(tmp, "copy.o")],
                       capture_output=True)
    if r.returncode != 0:          # a host-only object (no device code)
        return None
    subprocess.check_call([f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", f"--input={fat}",
                           "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={dev}"])
    return dev


def _notes(dev):
    txt = subprocess.check_output([f"{LLVM}/llvm-readelf", "--notes", dev], text=True)
    out = {}
    for blk in txt.split("- .agpr_count:")[1:]:
        blk = ".agpr_count:" + blk
        g = lambda k: (re.search(r"\." + k + r":\s*(\S+)", blk) or [None, "?"])[1]  # noqa: E731
        out[g("name")] = "/".join(g(k) for k in ("vgpr_count", "agpr_count", "sgpr_count", "private_segment_fixed_size",
                                                  "group_segment_fixed_size"))
    return out


def _streams(dev):
    txt = subprocess.check_output([f"{LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", "--no-leading-addr", dev], text=True)
    out, cur = {}, None
    for line in txt.splitlines():
        m = re.match(r"^[0-9a-f]* ?<(.+)>:$", line.strip())
        if m:
            cur = m.group(1)
            out[cur] = []
            continue
        if cur is None or not line.strip() or line.strip().startswith(";"):
            continue
        ins = re.sub(r"\s*//.*$", "", line).strip()
        ins = re.sub(r"<[^>]*>", "", ins).strip()
        if ins:
            out[cur].append(ins)
    return out


def collect(d):
    kern, regs = {}, {}
    with tempfile.TemporaryDirectory() as tmp:
        for obj in sorted(glob.glob(os.path.join(d, "*.o"))):
            dev = _device_object(obj, tmp)
            if dev is None:
                continue
            n = _notes(dev)
            s = _streams(dev)
            for k in n:
                kern[k] = s.get(k, [])
                regs[k] = n[k]
    return kern, regs


def main():
    before, after = sys.argv[1], sys.argv[2]
    kb, rb = collect(before)
    ka, ra = collect(after)
    lines, same = [], 0
    for k in sorted(kb):
        if k in ka:
            ident = kb[k] == ka[k]
            same += ident
            lines.append(f"{k[:70]:70s} {rb[k]:>22s} {len(kb[k]):6d} | {ra[k]:>22s} {len(ka[k]):6d} | {'yes' if ident else 'NO'}")
        else:
            lines.append(f"{k[:70]:70s} {rb[k]:>22s} {len(kb[k]):6d} | {'(gone)':>29s} | NO")
    added = sorted(set(ka) - set(kb))
    summary = [f"kernels before: {len(kb)}, after: {len(ka)}; present in both with identical streams: {same} of {len(kb)}",
               "added: " + (", ".join(added) if added else "none")]
    text = "\n".join(lines + [""] + summary) + "\n"
    print(text)
    if len(sys.argv) > 3:
        with open(sys.argv[3], "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
