"""Compile-time guard on the ResBlock kernels compiled per dilation (rb_conv.h rb_group_dil_kernel, rb_pair.h rbp_dil_group_kernel):
they must cost no more registers, LDS or occupancy than the run-time-dilation kernels they stand in for, and never scratch.
(hipcc's kernel-resource-usage remarks, through test_kernel_resources.py's cache; no GPU.)"""
import re

import pytest

from tests.test_kernel_resources import resources  # noqa: F401  (the fixture)


def _one(table, pattern):
    hit = {n: r for n, r in table.items() if re.search(pattern, n)}
    assert len(hit) == 1, (pattern, sorted(hit))
    return next(iter(hit.values()))


@pytest.mark.parametrize("nb, vgprs, lds, occupancy", [(2, 128, 32 * 1024, 4), (4, 168, 48 * 1024, 3)])
def test_group_kernels_per_dilation(resources, nb, vgprs, lds, occupancy):  # noqa: F811
    base = _one(resources, rf"rb_group_kernelILi11ELi7ELi3ELi{nb}EEE")
    dil = {n: r for n, r in resources.items() if re.search(rf"rb_group_dil_kernelILi11ELi7ELi3ELi{nb}ELi\d+EEE", n)}
    assert sorted(int(re.search(r"Li(\d+)EEE", n).group(1)) for n in dil) == [1, 3, 5], sorted(dil)
    for n, r in dil.items():
        assert r["scratch"] == 0 and r["vgprs"] <= min(vgprs, base["vgprs"]) and r["occupancy"] >= occupancy, (n, r, base)
        assert r["lds"] == base["lds"] <= lds, (n, r, base)


@pytest.mark.parametrize("cb, lds", [(2, 47 * 1024), (1, 40 * 1024)])
def test_pair_kernels_per_dilation(resources, cb, lds):  # noqa: F811
    base = _one(resources, rf"rb_pair_group_kernelILi11ELi7ELi3ELi{cb}EEE")
    dil = {n: r for n, r in resources.items() if re.search(rf"rbp_dil_group_kernelILi11ELi7ELi3ELi{cb}ELi\d+EEE", n)}
    assert sorted(int(re.search(r"Li(\d+)EEE", n).group(1)) for n in dil) == [1, 3, 5], sorted(dil)
    for n, r in dil.items():
        assert r["scratch"] == 0 and r["vgprs"] <= min(168, base["vgprs"]) and r["occupancy"] >= 3, (n, r, base)
        assert r["lds"] == base["lds"] <= lds, (n, r, base)


def test_runtime_dilation_kernels_kept_their_registers(resources):  # noqa: F811
    """The scalar-base fragment loads reach the run-time-dilation kernels too: no more registers than before them (122 / 154 / 130)."""
    assert _one(resources, r"rb_group_kernelILi11ELi7ELi3ELi2EEE")["vgprs"] <= 122
    assert _one(resources, r"rb_group_kernelILi11ELi7ELi3ELi4EEE")["vgprs"] <= 154
    for cb in (1, 2):
        r = _one(resources, rf"rb_pair_group_kernelILi11ELi7ELi3ELi{cb}EEE")
        assert r["vgprs"] <= 132 and r["scratch"] == 0, r
