"""The three lane maps of the whole-line in-place residual epilogue (csrc/gemm_w4.hip, resid_tile_wl), as plain Python -- no GPU.

A wave owns 128 token rows x 128 features.  With the MFMA's operand roles swapped, lane (q, c) = (lane >> 4, lane & 15) holds features 8 c .. 8 c + 7
of token 16 j + 4 q + r per (token tile j, component r): the NEW map, in which the stream is loaded and stored (16 lanes = 256 contiguous bytes).
The partial row statistics keep the summation tree of the OLD map -- lane (fr, fq) = (lane & 15, lane >> 4) holds features 16 ii + 4 fq + e of token
fr + 16 j per 64-feature half h -- so a token tile's 16 x 128 packed fp16 values travel through a 4-KiB patch of LDS: written token-major with
ds_write_b128 (row t = token, logical 16-byte chunk c at physical chunk c ^ t), read back as the old map's 8-byte pieces with ds_read_b64.

(a) new map -> patch address -> old map is the identity on (token, feature) for all 64 lanes x 8 token tiles x 4 components;
(b) no wave access of either instruction puts two different addresses of one service group on one bank (LDS of CDNA4: ds_write_b128 is served in
    8 groups of 8 contiguous lanes over 32 banks of 4 bytes, ds_read_b64 in 2 groups of 32 lanes over 64 banks).

The address expressions below are the kernel's (wof / rof and the XOR immediates), restated, not re-derived."""
import itertools

PATCH_BYTES = 4096


def write_addr(lane, r):
    """byte address of the lane's ds_write_b128 of component r (16 bytes: features 8 c .. 8 c + 7 of token row 4 q + r)"""
    q, c = lane >> 4, lane & 15
    wof = 4 * q * 256 + ((c ^ (4 * q)) * 16)
    return (wof ^ (16 * r)) + 256 * r


def read_addr(lane, h, ii):
    """byte address of the lane's ds_read_b64 of piece (half h, feature tile ii): 4 fp16 = features 64 h + 16 ii + 4 fq .. + 3 of token row fr"""
    fr, fq = lane & 15, lane >> 4
    rof = fr * 256 + ((fr >> 1) & 7) * 32 + (((fq >> 1) ^ (fr & 1)) * 16) + (fq & 1) * 8
    return rof ^ (32 * (4 * h + ii))


def new_map(lane, j, r, i):
    """(token, feature) inside the wave's 128 x 128 of accumulator acc[i][j][r] of `lane`"""
    q, c = lane >> 4, lane & 15
    return 16 * j + 4 * q + r, 8 * c + i


def old_map(lane, j, h, ii, e):
    """(token, feature) of element e of the old map's piece (half h, feature tile ii) of token tile j"""
    fr, fq = lane & 15, lane >> 4
    return fr + 16 * j, 64 * h + 16 * ii + 4 * fq + e


def test_new_map_covers_the_wave_tile_once():
    seen = {new_map(lane, j, r, i) for lane in range(64) for j in range(8) for r in range(4) for i in range(8)}
    assert seen == set(itertools.product(range(128), range(128)))


def test_composition_is_the_identity():
    """(a) per token tile: what the new map writes into the patch is what the old map expects to read there"""
    for j in range(8):
        patch = {}
        for lane in range(64):
            for r in range(4):
                a = write_addr(lane, r)
                assert 0 <= a and a + 16 <= PATCH_BYTES and a % 16 == 0
                for i in range(8):
                    assert a + 2 * i not in patch  # (every fp16 slot of the patch written once)
                    patch[a + 2 * i] = new_map(lane, j, r, i)
        assert len(patch) == PATCH_BYTES // 2
        for lane in range(64):
            for h in range(2):
                for ii in range(4):
                    a = read_addr(lane, h, ii)
                    assert 0 <= a and a + 8 <= PATCH_BYTES and a % 8 == 0
                    for e in range(4):
                        assert patch[a + 2 * e] == old_map(lane, j, h, ii, e), (j, lane, h, ii, e)


def _conflicts(groups, addr_of, dwords, banks):
    """number of (group, bank) pairs that see two DIFFERENT dword addresses"""
    bad = 0
    for grp in groups:
        by_bank = {}
        for lane in grp:
            a = addr_of(lane)
            for d in range(dwords):
                w = a // 4 + d
                by_bank.setdefault(w % banks, set()).add(w)
        bad += sum(1 for ws in by_bank.values() if len(ws) > 1)
    return bad


def test_patch_accesses_are_bank_conflict_free():
    """(b)"""
    write_groups = [range(8 * g, 8 * g + 8) for g in range(8)]
    read_groups = [range(0, 32), range(32, 64)]
    for r in range(4):
        assert _conflicts(write_groups, lambda lane: write_addr(lane, r), 4, 32) == 0, r
    for h in range(2):
        for ii in range(4):
            assert _conflicts(read_groups, lambda lane: read_addr(lane, h, ii), 2, 64) == 0, (h, ii)


def test_the_checker_sees_an_unswizzled_patch():
    """the same model on the plain token-major image (chunk c at chunk c): the 16 rows of a read group share their banks"""
    plain_read = lambda lane, h, ii: (lane & 15) * 256 + (2 * (4 * h + ii) + (lane >> 5)) * 16 + ((lane >> 4) & 1) * 8
    assert _conflicts([range(0, 32), range(32, 64)], lambda lane: plain_read(lane, 0, 0), 2, 64) > 0


def test_row_mask_bits_in_the_new_map():
    """rowbits: byte [m / 128][m % 16], bit (m % 128) / 16.  The new map's lane reads the four bytes 4 q .. 4 q + 3 of its 128-row group as one dword;
    bit 8 r + j of it is the keep flag of token 16 j + 4 q + r."""
    import random
    rnd = random.Random(5)
    keep = [rnd.random() < 0.7 for _ in range(128)]
    rowbits = [sum(int(keep[16 * t + b]) << t for t in range(8)) for b in range(16)]
    for lane in range(64):
        q = lane >> 4
        kb4 = sum(rowbits[4 * q + r] << (8 * r) for r in range(4))
        for j in range(8):
            for r in range(4):
                assert bool((kb4 >> (8 * r + j)) & 1) == keep[new_map(lane, j, r, 0)[0]]
