"""Inputs of the diversity tests (tests/test_div_cpu.py, test_div_gpu.py, div_guard_child.py): the boundary shapes of the
k_div_* kernels - row words on both sides of a word seam, rows that need a second step of a lane group (WP = 33) and rows
that leave the registers (WP = 129), group counts on both sides of the 4-group tile, symbols and windows at their edges.
TEST INFRASTRUCTURE, never imported by edsparser_amd/."""
import random

from dist_cases import render
from ld_cases import biallelic_eds, panel_eds, wide_symbol_eds


def _req(**kw):
    return kw


def split(P, G, leave=0):
    """G groups of consecutive paths over 1..P - leave"""
    n = P - leave
    return [list(range(1 + n * g // G, 1 + n * (g + 1) // G)) for g in range(G)]


def edge_symbols_eds():
    """six paths; in order: a universal string behind an explicit one, a lone string that names only some paths, a symbol
    that leaves out the paths 4..6 (one group's only), two strings of equal text, a fixed stretch of 40 columns, a symbol of
    three strings and a trailing zero-width choice symbol"""
    syms = [[b"A", b"C"], [b"GG"], [b"T", b"TA"], [b"A", b"A"], [b"ACGTACGTAC" * 4], [b"A", b"C", b"G"], [b"", b""]]
    sets = [{1, 4}, {0}, {1, 2, 5}, {1, 2}, {3}, {1, 2, 4}, {3, 5, 6}, {0}, {1, 2}, {3, 4}, {5, 6}, {1, 2, 3}, {4, 5, 6}]
    return render(syms, sets)


def boundary_shapes():
    """name -> (eds, seds, requests): a request is the keyword arguments of PathSession.diversity / div_spec.diversity"""
    rng = random.Random(41)
    shapes = {}
    for P in (64, 65, 128, 129, 300):                            # path 64: bit 63 of word 0; path 65: bit 0 of word 1; WP = 3, 5
        groups3 = [list(range(1, P // 2)), [P // 2], list(range(P // 2 + 2, P + 1))]       # a group of one path; P / 2 + 1 left out
        shapes["paths%d" % P] = panel_eds(rng, P, 12, p_missing=0.1) + ([
            _req(sfs=True), _req(groups=split(P, 2, leave=3), size=4, step=2, sfs=True), _req(groups=groups3, unit="columns", size=7, sfs=True),
            _req(groups=[[P, 64, 1, 1], [63, 2] + ([65] if P > 65 else [])], size=5)],)
    big = [list(range(1, 1025)), list(range(1025, 2050))]
    shapes["paths2049"] = panel_eds(rng, 2049, 5, p_missing=0.02, fixed_every=0) + ([             # WP = 33: two steps of 32 lanes
        _req(sfs=True), _req(groups=big, size=2, sfs=True), _req(groups=[[2049], [1, 64, 65, 2048], list(range(100, 1500))], sfs=True)],)
    e, s = panel_eds(rng, 8200, 2, p_missing=0.01, fixed_every=0)                                  # WP = 129: the walk rows in HBM
    shapes["paths8200"] = (e, s, [_req(groups=[list(range(1, 200)), list(range(8000, 8201)), [4097], list(range(4000, 4090)),
                                              list(range(6000, 6300))], sfs=True),
                                  _req(groups=[list(range(1, 3000))], size=1, sfs=True)])
    shapes["groups16"] = panel_eds(rng, 70, 14, p_missing=0.1, universal="middle") + ([           # 6 paths left out; padding bits of word 1
        _req(groups=split(70, 16, leave=6), size=3, sfs=True), _req(groups=split(70, 5), unit="columns", size=10, step=4, sfs=True),
        _req(groups=split(70, 8, leave=1), sfs=True), _req(sfs=True)],)
    for where in ("first", "last"):
        shapes["universal_" + where] = panel_eds(rng, 70, 9, p_missing=0.2, universal=where) + ([_req(sfs=True, size=2),
                                                                                                   _req(groups=split(70, 3), sfs=True)],)
    shapes["edges"] = edge_symbols_eds() + ([_req(sfs=True), _req(groups=[[1, 2, 3], [4, 5, 6]], sfs=True),
                                             _req(groups=[[1, 2, 3], [4, 5, 6]], unit="columns", size=8, sfs=True),   # windows without a symbol
                                             _req(groups=[[6], [1, 2]], unit="columns", size=1), _req(unit="columns"),
                                             _req(unit="columns", size=1000), _req(unit="columns", size=5, step=11)],)
    shapes["wide70"] = wide_symbol_eds(rng) + ([_req(sfs=True), _req(groups=split(80, 4), size=10, sfs=True)],)
    eds, seds = panel_eds(rng, 20, 9, fixed_every=0)             # nc = 10
    shapes["windows"] = (eds, seds, [_req(size=z, step=t, groups=g) for g in (None, split(20, 2)) for z, t in
                                     ((1, 0), (10, 0), (11, 0), (25, 0), (3, 1), (3, 2), (2, 5), (4, 3), (0, 7), (10, 9))])
    e, s = biallelic_eds(rng, 4500, P=7)                         # 18 workgroups of 256 symbols, three scan tiles, a ragged last wave
    shapes["many"] = (e, s, [_req(groups=[[1, 2, 3], [4, 5, 6, 7]], size=100, step=50, sfs=True), _req(size=2048, sfs=True),
                             _req(unit="columns", size=64, step=512)])
    shapes["fixed"] = (b"{ACGT}{GG}{}", b"{0,3}{0}{0,1}", [_req(sfs=True), _req(unit="columns", size=2, groups=[[1], [2, 3]])])
    return shapes
