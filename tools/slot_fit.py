#!/usr/bin/env python3
"""How many waves per SIMD a kernel places in a slot that a streamed align launch leaves free (DESIGN.md sections 4.2b, 4.3).

usage: tools/slot_fit.py <hipcc -Rpass-analysis=kernel-resource-usage log> [name regex]

Two kinds of slot, both a CU shared with the launch's own workgroups (one wave per SIMD each):
  lean     a third of a CU, beside two workgroups of the lean exact DIRECT7 body: 168 VGPRs and 45,568 B of LDS each,
           so 512 - 2 * 168 = 176 VGPRs per SIMD and 163,840 - 2 * 45,568 = 72,704 B of LDS are free
  half-CU  half of a CU, beside one workgroup of a two-wave body (256 VGPRs, 45,568 B): 256 VGPRs per SIMD and 118,272 B free
A block of T threads puts ceil(T / 256) waves on every SIMD; registers are allocated in granules of 8 (AGPRs come out of the same 512);
a SIMD holds 8 waves.  The compiler's remarks do not carry the block size: 256 unless THREADS below (or name=threads on the command
line) says otherwise.
"""
import re
import subprocess
import sys

SIMD_VGPRS, CU_LDS, SIMD_WAVES, VGPR_GRANULE = 512, 163840, 8, 8
LEAN_VGPRS, LEAN_LDS = 168, 45568               # k_align_async<false, 7, ORD, true>
SLOTS = {                                         # name: (free VGPRs per SIMD, free LDS bytes, waves per SIMD the launch itself holds)
    "lean": (SIMD_VGPRS - 2 * LEAN_VGPRS, CU_LDS - 2 * LEAN_LDS, 2),
    "half-CU": (SIMD_VGPRS - 256, CU_LDS - LEAN_LDS, 1),
}
THREADS = {r"k_rs_scan<1[01]>": 1024, r"k_rank": 512, r"k_word_offsets": 1024, r"k_griddesc": 64}


def parse(text):
    """{mangled kernel name: {remark: value}} of a kernel-resource-usage log."""
    rows, cur = {}, None
    for line in text.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
            rows[cur] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z][\w /\[\]]*?): (\d+)", line)
        if m and cur:
            rows[cur][m.group(1).strip()] = int(m.group(2))
    return rows


def demangle(names):
    out = subprocess.run(["c++filt"] + list(names), capture_output=True, text=True).stdout.splitlines() if names else []
    return [re.sub(r"^void ", "", re.sub(r"\(.*", "", d)) for d in out]


def threads_of(short, extra=()):
    for pat, t in list(extra) + list(THREADS.items()):
        if re.search(pat, short):
            return t
    return 256


def waves_in_slot(res, slot, threads=256):
    """Waves per SIMD that blocks of `threads` threads with the resources `res` place in a slot of kind `slot`."""
    free_vgprs, free_lds, held = SLOTS[slot]
    per_block = -(-threads // 256)               # waves on each SIMD per block
    regs = -(-(res.get("VGPRs", 0) + res.get("AGPRs", 0)) // VGPR_GRANULE) * VGPR_GRANULE
    blocks = min(free_vgprs // max(regs * per_block, 1), (SIMD_WAVES - held) // per_block)
    lds = res.get("LDS Size [bytes/block]", 0)
    if lds:
        blocks = min(blocks, free_lds // lds)
    return blocks * per_block


def main():
    rows = parse(open(sys.argv[1]).read())
    pat, extra = None, []
    for a in sys.argv[2:]:
        if re.fullmatch(r".+=\d+", a):
            extra.append((a.rsplit("=", 1)[0], int(a.rsplit("=", 1)[1])))
        else:
            pat = re.compile(a)
    names = list(rows)
    print(f"{'kernel':44s} {'threads':>7s} {'VGPRs':>6s} {'scratch':>8s} {'LDS/block':>10s} {'lean slot':>10s} {'half-CU slot':>13s}   (waves per SIMD)")
    for n, short in zip(names, demangle(names)):
        if pat and not pat.search(short):
            continue
        r, t = rows[n], threads_of(short, extra)
        print(f"{short[:44]:44s} {t:7d} {r.get('VGPRs', -1) + r.get('AGPRs', 0):6d} {r.get('ScratchSize [bytes/lane]', -1):8d} {r.get('LDS Size [bytes/block]', -1):10d} "
              f"{waves_in_slot(r, 'lean', t):10d} {waves_in_slot(r, 'half-CU', t):13d}")


if __name__ == "__main__":
    main()
