#!/usr/bin/env python3
"""LDS bank-conflict model of fft_line8<.., ODD = 1> (k_solver.hip) for 16-byte elements: per stage, the mean conflict degree of its 128-bit reads
and writes. ds_write_b128 is served in groups of 8 consecutive lanes over 8 slots of 16 B, ds_read_b128 in the four 16-lane groups
{0-3,12-15,20-27}, {4-11,16-19,28-31}, +32 over 16 slots; lanes that read the same address count once. Lanes = threadIdx.x = line * T + t, element i
of a line at line * ld + lpad(i).   python tools/lds_odd_model.py [N ...]"""
import sys

lpad = lambda i: i + (i >> 3)
RGROUPS = [[0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27], [4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31]]
RGROUPS += [[l + 32 for l in g] for g in RGROUPS]
WGROUPS = [list(range(8 * g, 8 * g + 8)) for g in range(8)]


def degree(addr, groups, slots):      # addr: one address or None per lane of a wave
    worst = []
    for g in groups:
        per = {}
        for l in g:
            if l < len(addr) and addr[l] is not None:
                per.setdefault(addr[l] % slots, set()).add(addr[l])
        if per:
            worst.append(max(len(s) for s in per.values()))
    return worst


def stages(N):
    T = N // 8
    r = T
    while r % 2 == 0:
        r //= 2
    out = []      # (name, reads, writes): lists of functions t -> index or None, one per instruction
    Ns = 1
    for R in ([5] if r == 5 else [3, 3] if r == 9 else [3] if r == 3 else []):
        M, NB = N // R, (8 + R - 1) // R
        rd = [(lambda t, b=b, q=q, M=M: t + b * T + q * M if t + b * T < M else None) for b in range(NB) for q in range(R)]
        wr = [(lambda t, b=b, q=q, M=M, R=R, Ns=Ns: ((t + b * T) - (t + b * T) % Ns) * R + (t + b * T) % Ns + q * Ns if t + b * T < M else None) for b in range(NB) for q in range(R)]
        out.append((f"radix {R}, Ns {Ns}", rd, wr)); Ns *= R
    while Ns * 8 <= N:
        rd = [(lambda t, q=q: t + q * T) for q in range(8)]
        wr = [(lambda t, q=q, Ns=Ns: (t - t % Ns) * 8 + t % Ns + q * Ns) for q in range(8)]
        out.append((f"radix 8, Ns {Ns}", rd, wr)); Ns *= 8
    if Ns < N:
        R = N // Ns; NB = 8 // R; M = N // R
        rd = [(lambda t, b=b, q=q, M=M: t + b * T + q * M) for b in range(NB) for q in range(R)]
        wr = [(lambda t, b=b, q=q, R=R, Ns=Ns: ((t + b * T) - (t + b * T) % Ns) * R + (t + b * T) % Ns + q * Ns) for b in range(NB) for q in range(R)]
        out.append((f"radix {R}, Ns {Ns}", rd, wr))
    return out


def model(N, ld, threads):
    T = N // 8
    res = []
    for name, rd, wr in stages(N):
        row = [name]
        for fns, groups, slots in ((rd, RGROUPS, 16), (wr, WGROUPS, 8)):
            degs = []
            for f in fns:
                for w0 in range(0, threads, 64):
                    addr = []
                    for lane in range(w0, min(w0 + 64, threads)):
                        i = f(lane % T)
                        addr.append(None if i is None else (lane // T) * ld + lpad(i))
                    degs += degree(addr, groups, slots)
            row.append(sum(degs) / len(degs)); row.append(max(degs))
        res.append(row)
    return res


if __name__ == "__main__":
    for N in [int(a) for a in sys.argv[1:]] or [96, 384]:
        T = N // 8
        xthreads = T if T >= 256 else (256 // T) * T
        CB = max(1, min(max(8, 256 // T), 512 // T)); CB = CB // 8 * 8 if CB >= 8 else 4
        for what, ld, threads in (("x rows (pitch lpad(N) + 2)", lpad(N) + 2, xthreads), ("y lines (pitch lpad(N) + 1)", lpad(N) + 1, CB * T)):
            print(f"N = {N}, {what}, {threads} threads")
            for name, rm, rx, wm, wx in model(N, ld, threads):
                print(f"  {name:16s} reads: mean {rm:.2f} max {rx}   writes: mean {wm:.2f} max {wx}")
