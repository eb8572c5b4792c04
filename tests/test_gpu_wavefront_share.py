"""The trace / shade kernel pair on the edge-case scenes (tests/edge_scenes.py): the smallest scenes at which what the pair shares
with the single kernel (shade_common.h: lane_reset, finish_sample, flush_counters, nearest_plane) can go wrong -- planes and no
primitive at all (root_ref == REF_NONE: every ray is answered by nearest_plane alone), no plane, a single primitive, no light, a
point light.  Frame and counters against the oracle's mirror of the wavefront path, exactly as run_case checks the single kernel.
A pool of 512 slots is one shade block: on a 64 x 48 frame at 4 spp every slot is refilled about two dozen times."""
import pytest

import edge_scenes
from gpu_case import run_case

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("spp", [0, 4])
@pytest.mark.parametrize("name", list(edge_scenes.ALL))
def test_wavefront_pair_matches_oracle_on_edge_scene(name, spp):
    st, img = run_case(edge_scenes.ALL[name](), 64, 48, spp, wavefront=1, wf_pool=512)
    if name == "empty":
        assert img.max() == 0
    if name in ("plane_only", "single_sphere", "no_light", "bulbs_and_planes"):
        assert img[..., 3].max() == 255
