"""Do two builds of the library hold the same gfx950 device code?  Per kernel symbol, since instantiation order may move.
usage: python tools/compare_device_code.py <libmodppl_hip.so A> <libmodppl_hip.so B>
Unbundles every code object as tools/disasm_kernel.py does and compares, symbol by symbol, the instruction stream (mnemonics, operands
and encodings; load addresses and the <symbol+offset> labels objdump prints next to branches are dropped).  The one position-dependent
literal, the displacement `s_add_u32` adds to a fresh `s_getpc_b64`, is replaced by the symbol + offset it reaches in its own code
object, so a table or a callee that the linker merely placed elsewhere compares equal and another target does not.  Exit status 1 on a
difference."""
import bisect
import hashlib
import re
import subprocess
import sys
import tempfile
from pathlib import Path

LLVM = "/opt/rocm/lib/llvm/bin"


def kernels(lib):
    """{symbol: (instructions, sha256 of the normalised body)} over every code object of `lib`"""
    out = {}
    with tempfile.TemporaryDirectory() as td:
        td = Path(td)
        fat = td / "fat.bin"
        subprocess.run(["objcopy", "-O", "binary", "--only-section=.hip_fatbin", str(lib), str(fat)], check=True)
        blob = fat.read_bytes()
        starts = [m.start() for m in re.finditer(b"__CLANG_OFFLOAD_BUNDLE__", blob)]
        for i, s in enumerate(starts):
            part, co = td / f"b{i}.bin", td / f"d{i}.co"
            part.write_bytes(blob[s:starts[i + 1] if i + 1 < len(starts) else len(blob)])
            subprocess.run([f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", f"--input={part}",
                            "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}"], check=True)
            text = subprocess.run([f"{LLVM}/llvm-objdump", "-d", str(co)], capture_output=True, text=True, check=True).stdout
            table = subprocess.run([f"{LLVM}/llvm-objdump", "-t", str(co)], capture_output=True, text=True, check=True).stdout
            syms = sorted({(int(w[0], 16), w[-1]) for w in (ln.split() for ln in table.splitlines()) if len(w) >= 4 and re.fullmatch(r"[0-9a-f]{16}", w[0]) and "*UND*" not in w})
            addrs = [a for a, _ in syms]
            heads = list(re.finditer(r"^[0-9a-f]+ <([^>]+)>:\n", text, re.M))
            for k, m in enumerate(heads):
                body = text[m.end():heads[k + 1].start() if k + 1 < len(heads) else len(text)]
                # "\tinsn operands   // 000000001234: ENCODING <sym+0x10>"  ->  "insn operands // ENCODING"
                raw = [ln for ln in body.splitlines() if ln.strip() not in ("", "...")]   # ("...": zero padding up to the next symbol)
                lines = [re.sub(r"//\s*[0-9A-Fa-f]+:", "//", re.sub(r"\s*<[^>]+>\s*$", "", ln)).split() for ln in raw]
                for j in range(1, len(lines)):   # s_getpc_b64 s[a:b] // ADDR: ENC ; s_add_u32 sa, sa, DISP: the target is ADDR + 4 + DISP
                    if lines[j - 1][0] == "s_getpc_b64" and lines[j][0] == "s_add_u32":
                        pc = int(re.search(r"//\s*([0-9A-Fa-f]+):", raw[j - 1]).group(1), 16) + 4
                        target = (pc + int(lines[j][3], 16)) & 0xFFFFFFFF
                        at = bisect.bisect_right(addrs, target) - 1
                        lines[j] = lines[j][:3] + [f"{syms[at][1]}+{target - syms[at][0]:#x}"]
                norm = "\n".join(" ".join(w) for w in lines)
                assert (i, m.group(1)) not in out
                out[(i, m.group(1))] = (len(lines), hashlib.sha256(norm.encode()).hexdigest())
    return out


def main():
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    only_a, only_b = sorted(set(a) - set(b)), sorted(set(b) - set(a))
    differ = sorted(k for k in set(a) & set(b) if a[k] != b[k])
    print(f"code objects: {len({k[0] for k in a})} and {len({k[0] for k in b})}; symbols: {len(a)} and {len(b)}; "
          f"instructions: {sum(v[0] for v in a.values())} and {sum(v[0] for v in b.values())}")
    print(f"only in A: {len(only_a)}  only in B: {len(only_b)}  same symbol, different code: {len(differ)}")
    for k in only_a + only_b + differ:
        print("  ", k)
    sys.exit(1 if only_a or only_b or differ else 0)


if __name__ == "__main__":
    main()
