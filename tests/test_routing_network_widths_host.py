"""The network shapes of the routing device tests without a GPU (tests/routing_kinematic_cases.py: networks): at every size from 63
cells up and with every seed that the chained-call tests of tests/test_gpu_routing*.py pass, the shapes are networks that
elmk_routing_enable accepts and the widths of their upstream maps are all four that with_npad (k_routing.hip) can pick, so that a
change to a generator cannot lose an instantiation of k_routing_step or k_kinematic_step from the device tests unseen."""
import numpy as np
import pytest

from elmkernels_amd import routing as rt
from tests.routing_kinematic_cases import networks, tree, widths

# module of the chained-call test -> (its sizes from 63 cells up, the seed it passes at ncells cells)
CHAINED = {"routing": ((63, 64, 65, 257, 1001), 50), "kinematic": ((63, 64, 65, 257, 1001), 50), "inundation": ((63, 64, 65, 257, 1001), 52),
           "reservoir": ((64, 65, 257, 1001), 52), "heat": ((1001,), 52)}  # (the heat test runs every shape at 1001 cells only)
NAMES = ("outlets", "chain", "reverse", "eight", "forest", "binary", "quad")


@pytest.mark.parametrize("module", list(CHAINED))
def test_the_shapes_give_every_width(module):
    sizes, seed0 = CHAINED[module]
    for n in sizes:
        nets = networks(n, seed0 + n)
        assert tuple(nets) == NAMES  # (the two trees after the forest: they draw nothing, so the shapes before them are what they were)
        for name, down in nets.items():
            assert down.dtype == np.int32 and down.shape == (n,), (n, name)
            rt.check_network(down)
        assert widths(nets) == {1, 2, 4, 8}, (n, widths(nets))
        assert widths({k: nets[k] for k in ("outlets", "chain", "reverse")}) == {1} and widths({"eight": nets["eight"]}) == {8}
        assert widths({"binary": nets["binary"]}) == {2} and widths({"quad": nets["quad"]}) == {4}
        assert widths({"forest": nets["forest"]}) <= {4, 8}


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 64, 65, 257, 513, 1001])
def test_the_trees(n):
    """The two trees at their smallest sizes and across a workgroup: in-degrees by count, and the upstream cells of cell i by value."""
    nets = networks(n, 7)
    assert ("binary" in nets) == (n >= 3) and ("quad" in nets) == (n >= 5)
    for name, k in (("binary", 2), ("quad", 4)):
        if name not in nets:
            continue
        down = nets[name]
        assert np.array_equal(down, tree(n, k)) and down[0] == -1 and np.array_equal(down[1:], (np.arange(1, n) - 1) // k)
        rt.check_network(down)
        up = rt.upstream_map(down)
        deg = (up >= 0).sum(axis=0)
        assert deg.max() == k and rt.npad_of(up) == k
        i = np.arange(n)
        for slot in range(k):
            child = k * i + 1 + slot
            assert np.array_equal(up[slot], np.where(child < n, child, -1).astype(np.int32))
        far = (i >= 256 // k) & (up[0] >= 0)  # the cells whose upstream cells lie in another workgroup of 256 cells than they do
        assert (up[0][far] // 256 > i[far] // 256).all() and far.any() == (n >= 258)
    # the shapes before the trees do not depend on them: the generator's draws are the forest's alone
    if n >= 3:
        assert np.array_equal(nets["forest"], networks(n, 7)["forest"])
