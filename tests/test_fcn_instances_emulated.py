"""CPU: the table of tests/fcn_instance_checks.py reaches every kernel instance lm_g2_launch holds (no library needed), and -- on the
emulated build of the HIP sources -- four of its configurations with their plain twins at 33x40, the refusals of formats without an instance.
The emulator has no register budget, LDS-DMA ring or barrier to get wrong: what it checks is the host side (recipes, weight packing,
row_channel, slice tables) and the kernel's index arithmetic per instance; the device run of the whole table is tests/test_fcn_instances_gpu.py.
An emulated forward pass of these networks takes 7-20 s; the module 110 s in all (eight cores)."""
import pytest

import fcn_instance_checks as ic
from test_fcn2_instances import dispatcher_instances

# each (KH, KW, EPI) family, 16 x 32 tiles, the loader wave, several channel tiles, all four formats
EMULATED = ("x3-wide", "x1-loader", "x4-loader", "x2-loader")
SIZE = (33, 40)


def test_table_reaches_every_instance():
    """the union of the table's instances is exactly the dispatcher's list; every configuration is needed; the engine's knobs choose the
    same instances at every tested size; every instance with a variant or several channel tiles occurs where the plain twins walk K alike;
    the all-f16x3 configurations hold every TERMS = 3 instance"""
    have, cfgs = dispatcher_instances(), ic.configurations()
    assert len(cfgs) <= 16 and len(set(c.name for c in cfgs)) == len(cfgs)
    per, exact = {}, set()
    for c in cfgs:
        ic.check_requests_honoured(c)
        per[c.name] = set(ic.instances(c).values())
        for size in (SIZE, (67, 131)):
            assert ic.instances(c, *size) == ic.instances(c) and ic.walk(c, *size) == ic.walk(c), (c.name, size)
        for l, r in ic.recipes(c).items():
            assert r.lds_bytes <= 160 * 1024, (c.name, l, r.lds_bytes)
        if all(ic.walk(t) == ic.walk(c) for _, t in ic.twins(c)):
            exact |= per[c.name]
        for _, t in ic.twins(c):            # a twin runs base instances the library holds
            assert set(ic.instances(t).values()) <= have, t.name
    union = set().union(*per.values())
    assert union == have, "instances no configuration runs: %s; instances the dispatcher does not hold: %s" % (sorted(have - union), sorted(union - have))
    for name in per:
        rest = set().union(*(v for k, v in per.items() if k != name))
        assert rest != have, "configuration %s adds no instance" % name
    loose = sorted(i for i in have if ic.is_variant(i) and i not in exact)
    assert not loose, "variant instances that never meet a twin with the same K walk: %s" % loose
    split = set().union(*(per[c.name] for c in cfgs if ic.all_f16x3(c)))
    assert sorted(i for i in have if i[2] == 3 and i not in split) == [] and sum(i[2] == 3 for i in have) == 20
    # the emulated choice: every family, 16 x 32 tiles, the loader wave, several channel tiles
    emu = set().union(*(per[n] for n in EMULATED))
    assert set((i[0], i[1], i[4]) for i in emu) == set((i[0], i[1], i[4]) for i in have)
    assert any(i[5] == 2 for i in emu) and any(i[6] == 1 for i in emu) and any(i[3] > 1 for i in emu)


@pytest.mark.parametrize("name", EMULATED)
def test_configuration_vs_oracle_and_twins(emu_lib, monkeypatch, name):
    cfg = {c.name: c for c in ic.configurations()}[name]
    ic.check_config(emu_lib, cfg, *SIZE, monkeypatch)


def test_formats_without_an_instance_are_refused(emu_lib):
    ic.check_refusals(emu_lib)
