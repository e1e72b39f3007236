"""Static check of the kernels' argument heads (kernarg preload).  No GPU needed.

From a built library: the gfx950 code object (the .hip_fatbin section, unbundled with clang-offload-bundler), its kernel
descriptors and instructions (llvm-objdump -d), and per kernel symbol
  preload  the descriptor's kernarg preload length in dwords (user SGPRs the command processor fills before the wave starts);
  waited   how many scalar loads based on the kernarg segment pointer are waited for (an s_waitcnt with an lgkmcnt term) before the
           first vector memory load of the body.  The body starts at the 256-byte block behind the compatibility prologue that a
           kernel with preloaded arguments carries (firmware that does not preload enters there and loads the same SGPRs itself).
Only load and wait mnemonics are matched, and the scalar moves and adds that carry the kernarg pointer on.  "Based on the kernarg
segment pointer" means: on the user SGPR pair the descriptor assigns to it, on an s_mov_b64 copy of such a pair, or on a pair made from
one by s_add_u32 / s_addc_u32 (a pointer into the segment).  A pointer that reached its register pair any other way (through a VGPR and
v_readfirstlane, say) is not followed: the compiler has no reason to do that with a uniform argument pointer, and
tests/test_kernarg_heads.py holds the count against the plain build, where it must not be 0.

    python tools/kernarg_heads.py toyslam_amd/libtsgo_hip.so [base name ...]
"""
import collections
import os
import re
import shutil
import subprocess
import sys
import tempfile

TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
# launched once per PCG iteration or once per Gauss-Newton step (engine/engine_launch.inc, engine_solve.inc)
HOT_KERNELS = ("k_schur_lm", "k_schur_pose", "k_restrict", "k_bcsr_residual", "k_bcsr_apply", "k_prolong_add", "k_rowdot_wg", "k_tail_up",
               "k_bottom_apply", "k_coarse_tail", "k_dense_apply", "k_smooth0", "k_iter_gate", "k_cg_step", "k_cg_update", "k_fold_partials",
               "k_lin_lm", "k_lin_pose", "k_pose_finalize", "k_pack_x", "k_warm_residual", "k_warm_scale", "k_save_x", "k_pose_update")

Head = collections.namedtuple("Head", "symbol base preload waited first_load")


def _llvm(tool):
    for d in (os.environ.get("ROCM_PATH", "/opt/rocm") + "/llvm/bin", "/opt/rocm/llvm/bin"):
        if os.path.exists(os.path.join(d, tool)):
            return os.path.join(d, tool)
    p = shutil.which(tool)
    if not p:
        raise RuntimeError("kernarg_heads: %s not found" % tool)
    return p


def base_name(symbol):
    """The function's own name out of an Itanium-mangled symbol: _Z7k_plainI...E -> k_plain, _ZN4tsgo10k_schur_lmI...E -> k_schur_lm."""
    if not symbol.startswith("_Z"):
        return symbol
    s, name = symbol[2:], None
    if s.startswith("N"):
        s = s[1:]
    while True:
        m = re.match(r"(\d+)", s)
        if not m:
            return name or symbol
        n = int(m.group(1))
        name = s[m.end():m.end() + n]
        s = s[m.end() + n:]


def code_object(lib, workdir):
    fat, co = os.path.join(workdir, "fat.bin"), os.path.join(workdir, "gfx950.co")
    subprocess.check_call([_llvm("llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, lib, os.path.join(workdir, "unused")])
    subprocess.check_call([_llvm("clang-offload-bundler"), "--unbundle", "--type=o", "--input=" + fat, "--targets=" + TARGET, "--output=" + co])
    return co


_SYM = re.compile(r"^[0-9a-f]+ <(.+)>:$")
_INS = re.compile(r"^\s+(\S+)\s*(.*?)\s*//\s*([0-9A-Fa-f]+):")


def descriptors(co):
    """symbol -> {directive: value} of every kernel descriptor (<symbol>.kd in .rodata)."""
    out, cur = {}, None
    for line in subprocess.check_output([_llvm("llvm-objdump"), "-d", "-j", ".rodata", co], text=True).splitlines():
        m = _SYM.match(line)
        if m:
            cur = out.setdefault(m.group(1)[:-3], {}) if m.group(1).endswith(".kd") else None
            continue
        f = line.split()
        if cur is not None and len(f) == 2 and f[0].startswith(".amdhsa_"):
            try:
                cur[f[0]] = int(f[1], 0)
            except ValueError:
                pass
    return out


def _regs(op):
    """SGPR numbers named by an operand: s5 -> {5}, s[4:7] -> {4..7}; anything else -> {}."""
    m = re.fullmatch(r"s(\d+)", op)
    if m:
        return {int(m.group(1))}
    m = re.fullmatch(r"s\[(\d+):(\d+)\]", op)
    return set(range(int(m.group(1)), int(m.group(2)) + 1)) if m else set()


def _head_of(ins, start, kd):
    preload = kd.get(".amdhsa_user_sgpr_kernarg_preload_length", 0)
    body = start + 256 if preload else start
    k0 = 4 * kd.get(".amdhsa_user_sgpr_private_segment_buffer", 0) + 2 * kd.get(".amdhsa_user_sgpr_dispatch_ptr", 0) + 2 * kd.get(".amdhsa_user_sgpr_queue_ptr", 0)
    kernarg = [{k0, k0 + 1}]          # SGPR pairs that hold the kernarg segment pointer, or a pointer into the segment
    pending = waited = 0
    low = None                        # destination of an s_add_u32 from the low half of such a pair: the s_addc_u32 behind it completes a pair
    for addr, op, args in ins:
        if addr < body:
            continue
        a = [x.strip() for x in args.split(",")] if args else []
        if op.startswith(("global_load", "flat_load", "buffer_load")):
            return preload, waited, op
        if op == "s_waitcnt" and "lgkmcnt" in args:
            waited += pending
            pending = 0
        elif op.startswith("s_load_dword") and len(a) >= 2 and _regs(a[1]) in kernarg:
            pending += 1
            kernarg = [p for p in kernarg if not (p & _regs(a[0]))]
        elif op == "s_mov_b64" and len(a) == 2 and _regs(a[1]) in kernarg:
            kernarg.append(_regs(a[0]))
        elif op == "s_add_u32" and len(a) == 3 and any(_regs(x) and min(p) in _regs(x) for p in kernarg for x in a[1:]):
            low = _regs(a[0])
        elif op == "s_addc_u32" and len(a) == 3 and low and _regs(a[0]) == {min(low) + 1} and any(_regs(x) and max(p) in _regs(x) for p in kernarg for x in a[1:]):
            kernarg = [p for p in kernarg if not (p & (low | _regs(a[0])))] + [low | _regs(a[0])]
            low = None
        elif op.startswith("s_") and a and not op.startswith(("s_cmp", "s_bitcmp", "s_waitcnt", "s_cbranch", "s_branch", "s_nop", "s_barrier")):
            kernarg = [p for p in kernarg if not (p & _regs(a[0]))]
    return preload, waited, None


def heads(lib, only=None):
    """A Head per kernel symbol of `lib` (only: the base names wanted; None: every kernel)."""
    with tempfile.TemporaryDirectory() as tmp:
        co = code_object(lib, tmp)
        kds = descriptors(co)
        text = subprocess.check_output([_llvm("llvm-objdump"), "-d", co], text=True)
    out, sym, start, ins = [], None, 0, []

    def close():
        if sym in kds and (only is None or base_name(sym) in only):
            out.append(Head(sym, base_name(sym), *_head_of(ins, start, kds[sym])))
    for line in text.splitlines():
        m = _SYM.match(line)
        if m:
            close()
            sym, start, ins = m.group(1), int(line.split()[0], 16), []
            continue
        m = _INS.match(line)
        if m and sym:
            ins.append((int(m.group(3), 16), m.group(1), m.group(2)))
    close()
    return out


def summary(hs):
    """base name -> (instantiations, smallest preload length, largest number of waited kernarg loads)."""
    out = {}
    for h in hs:
        n, p, w = out.get(h.base, (0, 1 << 30, 0))
        out[h.base] = (n + 1, min(p, h.preload), max(w, h.waited))
    return out


if __name__ == "__main__":
    names = set(sys.argv[2:]) or set(HOT_KERNELS)
    hs = heads(sys.argv[1], names)
    print("%-18s %5s %12s %12s" % ("kernel", "inst", "min preload", "max waited"))
    for b, (n, p, w) in sorted(summary(hs).items()):
        print("%-18s %5d %12d %12d" % (b, n, p, w))
    if os.environ.get("KERNARG_HEADS_VERBOSE"):
        for h in hs:
            if h.waited or not h.preload:
                print(h.symbol, h.preload, h.waited)
