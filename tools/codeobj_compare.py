"""Kernel by kernel comparison of two gfx950 code objects (the method of profiles/*_codeobj.txt): for a change
that must leave the device code alone.

    hipcc <_build.HIPCC_FLAGS without -shared -fPIC> --cuda-device-only --no-gpu-bundle-output -c X.hip -o X.elf
    python tools/codeobj_compare.py OLD.elf NEW.elf

Per kernel symbol (every FUNC with a .kd descriptor): size and sha256[:16] of its code bytes and its metadata block
of llvm-readelf --notes. Where the bytes differ at equal size, llvm-objdump -d of both, compared instruction by
instruction with literals masked. Exits non-zero unless every kernel is identical or differs in literals only."""
import hashlib
import os
import re
import subprocess
import sys

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/llvm/bin")


def run(tool, *args):
    return subprocess.run([os.path.join(LLVM, tool), *args], check=True, capture_output=True, text=True).stdout


def kernels(path):
    """{symbol: (code bytes, metadata text)}"""
    secs = {}  # index -> (address, file offset)
    for m in re.finditer(r"^\s*\[\s*(\d+)\]\s+\S*\s+\S+\s+([0-9a-f]+)\s+([0-9a-f]+)\s", run("llvm-readelf", "-S", "-W", path), re.M):
        secs[int(m.group(1))] = (int(m.group(2), 16), int(m.group(3), 16))
    syms = {}
    for ln in run("llvm-readelf", "-s", "-W", path).splitlines():
        f = ln.split()
        if len(f) == 8 and f[3] in ("FUNC", "OBJECT") and f[6].isdigit():
            syms[f[7]] = (int(f[1], 16), int(f[2]), int(f[6]), f[3])
    meta = {}
    for block in re.split(r"\n  - (?=\.)", run("llvm-readelf", "--notes", path)):
        m = re.search(r"\.symbol:\s+'?([^'\s]+)\.kd'?", block)
        if m:
            meta[m.group(1)] = re.sub(r"\namdhsa\.(target|version)[\s\S]*", "", block).strip()
    data = open(path, "rb").read()
    out = {}
    for name, (addr, size, sec, kind) in syms.items():
        if kind == "FUNC" and name + ".kd" in syms:
            off = secs[sec][1] + addr - secs[sec][0]
            out[name] = (data[off:off + size], meta.get(name, ""))
    return out


def disasm(path, sym):
    text = run("llvm-objdump", "-d", "--no-show-raw-insn", f"--disassemble-symbols={sym}", path)
    return [re.sub(r"\s*//.*", "", ln).strip() for ln in text.splitlines() if ln.startswith("\t")]


def main(old, new):
    a, b = kernels(old), kernels(new)
    print(f"# kernels: {os.path.basename(old)} {len(a)}, {os.path.basename(new)} {len(b)}")
    print(f"# only in old: {sorted(set(a) - set(b))}\n# only in new: {sorted(set(b) - set(a))}")
    print("# symbol | old size sha256[:16] | new size sha256[:16] | verdict")
    bad = len(set(a) ^ set(b))
    tally = {}
    for k in sorted(set(a) & set(b)):
        (ca, ma), (cb, mb) = a[k], b[k]
        if ca == cb and ma == mb:
            verdict = "identical"
        elif len(ca) == len(cb) and ma == mb:
            da, db = disasm(old, k), disasm(new, k)
            mask = lambda s: re.sub(r"0x[0-9a-f]+", "LIT", s)  # noqa: E731
            diff = [(x, y) for x, y in zip(da, db) if x != y]
            if len(da) == len(db) and all(mask(x) == mask(y) for x, y in diff):
                verdict = f"same size and metadata, {len(diff)} instruction(s) differ in a literal only"
                for x, y in diff:
                    print(f"#    {k}: '{x}' -> '{y}'")
            else:
                verdict, bad = "INSTRUCTIONS DIFFER", bad + 1
        else:
            verdict, bad = "DIFFERENT SIZE" if len(ca) != len(cb) else "METADATA DIFFERS", bad + 1
        tally[verdict.split(",")[0]] = tally.get(verdict.split(",")[0], 0) + 1
        h = lambda c: hashlib.sha256(c).hexdigest()[:16]  # noqa: E731
        print(f"{k} | {len(ca)} {h(ca)} | {len(cb)} {h(cb)} | {verdict}")
    print(f"# {tally}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(*sys.argv[1:3]))
