"""CPU: the kernel instances lm_fcn2.hip's dispatcher holds (the LM_G2_TRY lists of lm_g2_launch) and lecturemath_amd/fcn2.py: have_instance --
the table the recipes consult before they ask for a variant -- name the same set.  A variant only one of them knows is either a launch
that fails at run time or a kernel nobody can reach."""
import itertools
import os
import re

from lecturemath_amd import fcn2

SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "lecturemath_amd", "csrc", "lm_fcn2.hip")
EPI = {"LM_G2_EPI_PO": fcn2.EPI_PO, "LM_G2_EPI_T": fcn2.EPI_T, "LM_G2_EPI_TC": fcn2.EPI_TC, "LM_G2_EPI_V": fcn2.EPI_V}


def dispatcher_instances():
    text = open(SRC).read()
    body = text[text.index("static int lm_g2_launch(const LmF2Layer& l"):text.index("#undef LM_G2_TRY\n")]
    m77 = re.search(r"#define LM_G2_TRY77\(N, L\) \\\n(.*?)\n\s*LM_G2_TRY77\(", body, re.S)
    assert m77, "LM_G2_TRY77 not found"
    for n, l in re.findall(r"LM_G2_TRY77\((\d), (\d)\)", body[m77.end() - 12:]):
        body += "\n" + m77.group(1).replace("N, L)", "%s, %s)" % (n, l))
    out = set()
    for kh, kw, t, e, n, l in re.findall(r"LM_G2_TRY_MT4\((\d), (\d), (\d), (\w+), (\d), (\d)\)", body):
        for m in (1, 2, 3, 4):
            out.add((int(kh), int(kw), int(t), m, EPI[e], int(n), int(l)))
    for kh, kw, t, m, e, n, l in re.findall(r"LM_G2_TRY\((\d), (\d), (\d), (\d), (\w+), (\d), (\d)\)", body):
        out.add((int(kh), int(kw), int(t), int(m), EPI[e], int(n), int(l)))
    return out


def test_dispatcher_and_have_instance_agree():
    have = dispatcher_instances()
    assert len(have) > 60
    grid = set()
    for (kh, kw), epi in (((3, 3), fcn2.EPI_PO), ((1, 1), fcn2.EPI_TC), ((1, 7), fcn2.EPI_T), ((1, 7), fcn2.EPI_V), ((7, 7), fcn2.EPI_PO)):
        for terms, mt, nc, loader in itertools.product((1, 2, 3, 4), (1, 2, 3, 4), (1, 2), (0, 1)):
            if fcn2.have_instance(kh, kw, terms, mt, epi, nc, loader):
                grid.add((kh, kw, terms, mt, epi, nc, loader))
    assert grid == have, ("only in fcn2.have_instance: %s; only in lm_g2_launch: %s" % (sorted(grid - have), sorted(have - grid)))
    # the merged transposed convolution (EPI_TC2) launches the EPI_TC template with four channel tiles
    assert fcn2.have_instance(1, 1, 1, 4, fcn2.EPI_TC2) and (1, 1, 1, 4, fcn2.EPI_TC, 1, 0) in have


def test_tensor_table_agrees_with_lm_fcn2_create():
    """fcn2.TENSORS (id, pyramid level, which width is the channel count) against the LM_F2_* enum and the def(id, channels, level) calls of
    lm_fcn2_create; the T_* names against the enum; the array lengths of the C interface against N_TENSORS / N_LAYERS"""
    text = open(SRC).read()
    enum = {k: int(v) for k, v in re.findall(r"(LM_F2_\w+) = (\d+)", re.search(r"enum \{ (LM_F2_X0P = 0.*?) \};", text).group(1))}
    assert enum == {"LM_F2_" + k[2:]: getattr(fcn2, k) for k in ("T_X0P", "T_PRE0", "T_POOL0", "T_MID", "T_UPT0", "T_CU0", "T_XUP", "T_DP", "T_P1", "T_P2")}
    start = text.index("auto def = [&](int id, int channels, int level)")
    body = text[start:text.index("\n", text.index("def(LM_F2_P2,", start))]         # the lambda's own line, then one line per def or loop of defs

    class Widths:
        def __getitem__(self, i):
            return ("width", i)
    table = {}
    for line in body.splitlines()[1:]:
        loop = re.search(r"for \(int n = 0; n < (\d+); n\+\+\)", line)
        for n in range(int(loop.group(1)) if loop else 1):
            for tid, channels, level in re.findall(r"def\(([^,;]+), ([^,;]+), ([^,;)]+)\)", line):
                env = dict(enum, n=n, w=Widths())
                c = eval(channels, {}, env)
                assert c == 8 or isinstance(c, tuple), line
                tid = eval(tid, {}, env)
                assert tid not in table, line
                table[tid] = (eval(level, {}, env), None if c == 8 else c[1])
    assert table == {t.id: (t.level, t.width) for t in fcn2.TENSORS} and len(table) == fcn2.N_TENSORS == 25
    assert [t.id for t in fcn2.TENSORS] == list(range(fcn2.N_TENSORS)) and len(set(fcn2.TENSOR_NAMES.values())) == fcn2.N_TENSORS
    # derived views: every tensor takes an exponent exactly once (pooled copies through the tensor they are pooled from), fixed ones excepted
    groups = [t for o in fcn2.TENSOR_ORDER for t in fcn2.exponent_group(o)]
    assert sorted(groups) == list(range(fcn2.N_TENSORS)) and set(fcn2.FIXED_TENSORS) == {fcn2.T_X0P, fcn2.T_DP}
    assert all(fcn2.TENSORS[a].level == fcn2.TENSORS[b].level - 1 and fcn2.TENSORS[a].width == fcn2.TENSORS[b].width for a, b in map(fcn2.exponent_group, range(fcn2.T_PRE0, fcn2.T_POOL0)))
    assert int(re.search(r"#define LM_F2_TENSORS (\d+)", text).group(1)) == fcn2.N_TENSORS
    assert sorted(fcn2.LAYER_NAMES) == [l for l in range(fcn2.N_LAYERS) if l != fcn2.L_REC]
