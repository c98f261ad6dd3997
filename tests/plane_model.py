"""Host model of the reduction's plane form (GMSM_OPT_REDUCE_TAIL = 2; gmsm_quad.h: k_combine_we<PLANES>, k_plane_sums;
gmsm_group_host.h: fold_planes): the step machines of the device code and the Horner walk of the host, statement for
statement, over the groups of tests/combine_model.py (an element is an integer, infinity is None; Z or Z_r).

After the serial level a window has T pairs (S_t, W_t) and its total is  sum W_t + L sum_t t S_t.  With t = 64 blk + t':
    block:   A = sum S_t, M_l = sum {S_t : bit l of t' set} (l < 6), sum W_t                       - combine_we_planes
    window:  Wsum = sum_blk sumW, m_l = sum_blk M_l, h_l = sum {A_blk : bit l of blk set}           - plane_sums
    total  = Wsum + sum_l 2^(log2L + l) m_l + sum_l 2^(log2L + 6 + l) h_l                           - fold_planes
additions only on the device; every doubling is the host's."""
from combine_model import Z

N = 64  # pairs per combine block


def combine_we_planes(S, W, grp=Z):
    """the six summing steps of k_combine_we: returns the block's 8 records [A, M_0..M_5, sum W]"""
    S, W = list(S), list(W)
    assert len(S) == N and len(W) == N
    for s in range(1, 7):
        g = 32 >> (s - 1)
        loaded = []
        grp.at("combine1", "pairs", s)
        for q in range(N):
            G, i = q // g, q % g
            if G > s:
                continue
            if G == 0:
                l = s - 1
                loaded.append((S, (2 * i) << l, S[(2 * i) << l], S[(2 * i + 1) << l]))
            elif G < s:
                l = G - 1
                loaded.append((S, (2 * i + 1) << l, S[(2 * i + 1) << l], S[(2 * (i + g) + 1) << l]))
            else:
                loaded.append((W, i, W[i], W[i + g]))
        for arr, k, x, y in loaded:
            arr[k] = grp.add(x, y)
    return [S[0]] + [S[1 << l] for l in range(6)] + [W[0]]


def plane_sums(blocks, nq=64, grp=Z):
    """k_plane_sums over the 8-record blocks of one window, one workgroup of nq quads per plane:
    [Wsum, m_0..m_5, h_0..h_(H-1)]"""
    nb = len(blocks)
    H = (nb - 1).bit_length()
    NBP = 1 << H
    out = [None] * (7 + H)
    for p in range(8):
        P = [blocks[b][p] if b < nb else None for b in range(NBP)]
        for s in range(1, H + 1):
            g = NBP >> s
            nops = g if p else g * s
            for o0 in range(0, nops, nq):
                grp.at("planes", "sum", s)
                loaded = []
                for j in range(nq):
                    op = o0 + j
                    if op >= nops:
                        continue
                    G, i = op >> (H - s), op & (g - 1)
                    if p:
                        assert G == 0
                        x, y = i, i + g
                    elif G == 0:
                        l = s - 1
                        x, y = (2 * i) << l, (2 * i + 1) << l
                    else:
                        l = G - 1
                        assert l < s - 1
                        x, y = (2 * i + 1) << l, (2 * (i + g) + 1) << l
                    assert 0 <= x < NBP and 0 <= y < NBP
                    loaded.append((x, P[x], P[y]))
                dests = [x for x, _, _ in loaded]
                assert len(set(dests)) == len(dests), "two quads write one record"
                for x, vx, vy in loaded:
                    P[x] = grp.add(vx, vy)
        if p:
            out[0 if p == 7 else p] = P[0]
        else:
            for l in range(H):
                out[7 + l] = P[1 << l]
    return out


def fold_planes(planes, c, log2L, grp=Z):
    """GroupHost::fold_planes: planes[w] = the 7 + H sums of window w; one Horner walk from the top bit down. Returns
    (value, doublings, additions)."""
    nwin, NP = len(planes), len(planes[0])
    top = c * (nwin - 1) + log2L + NP - 2
    at = [[] for _ in range(top + 1)]
    for w in range(nwin):
        for i, v in enumerate(planes[w]):
            if v is not None:
                at[c * w + (0 if i == 0 else log2L + i - 1)].append(v)
    b = top
    while b >= 0 and not at[b]:
        b -= 1
    acc, dbls, adds = None, 0, 0
    while b >= 0:
        for v in at[b]:
            acc = grp.add(acc, v)
            adds += 1
        if b == 0:
            break
        nb = b - 1
        while nb > 0 and not at[nb]:
            nb -= 1
        if acc is not None:
            for _ in range(b - nb):
                acc = grp.dbl(acc)
                dbls += 1
        b = nb
    return acc, dbls, adds


def window_planes(S, W, grp=Z, nq=64):
    """the device part for one window: T pairs -> 7 + H plane sums"""
    T = len(S)
    blocks = []
    for lo in range(0, T, N):
        s, w = list(S[lo:lo + N]), list(W[lo:lo + N])
        pad = N - len(s)
        blocks.append(combine_we_planes(s + [None] * pad, w + [None] * pad, grp))
    assert len(blocks) <= 128
    return plane_sums(blocks, nq, grp)
