"""srt_host::Renderer and MultiRenderer called out of order or with a scene that cannot be flattened: every case is an error the
handle reports (HostError with the C++ message), after which the same handle goes on rendering.  Pins the state a Renderer keeps
between calls (the frame in flight, the resident scene, the pinned frame) on the smallest scene: the unit cube, 16 x 16, one light."""
import os

import numpy as np
import pytest

import scenes
from simple_raytracer_amd import build, host

CUBE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "assets", "unit_cube.obj")
W = H = 16


def test_collect_without_submit_is_an_error_on_any_machine():
    build.build_all()
    with pytest.raises(host.HostError, match="^Renderer::collect: nothing submitted$"):
        host.Renderer(0).collect(8, 8)


def cube_scene(turn, hierarchy=True):
    """'One Sample Cube for Testing' (scenes.one_cube) with the unit cube loaded from its OBJ file, sized for the small frame;
    (ObjectManager, light)."""
    T = host.Transformation
    inv = scenes._orbit_view(T, 100.0, 0.0, 0.0, 0.0)
    om = host.ObjectManager()
    om.loadObjFile(CUBE)
    for m in (T.scale(1.2, 1.2, 1.2), T.roty(T.radians(turn)), inv):       # at focal 400 and distance 100: about ten of the 16 pixels across
        om.transformTriangles(CUBE, m)
    if hierarchy:
        om.build_bvh(CUBE)
    return om, list(T.mul_vec4(inv, scenes.LIGHT_DEFAULT)[:3]) + [1.0]


@pytest.mark.gpu
def test_order_errors_leave_the_handle_usable():
    om, light = cube_scene(25.0)
    assert om.num_tris(CUBE) == 12
    r, second = host.Renderer(0), host.Renderer(0)
    want, n = second.render(om, W, H, light)
    assert 20 < n < W * H and want.shape == (H, W, 3)

    # submit twice: the second is refused, the first frame is still the one in flight
    r.submit(om, W, H, light)
    with pytest.raises(host.HostError, match="^Renderer::submit: "):
        r.submit(om, W, H, light)
    got, k = r.collect(W, H)
    assert k == n and np.array_equal(got, want)
    with pytest.raises(host.HostError, match="^Renderer::collect: nothing submitted$"):
        r.collect(W, H)

    # an object without a hierarchy: refused before anything reaches the device; repaired, the same handle renders it
    bare, light = cube_scene(40.0, hierarchy=False)
    with pytest.raises(host.HostError):
        r.submit(bare, W, H, light)
    with pytest.raises(host.HostError):
        r.render(bare, W, H, light)
    bare.build_bvh(CUBE)
    got, k = r.render(bare, W, H, light)
    want40, n40 = second.render(bare, W, H, light)
    assert k == n40 and n40 > 20 and np.array_equal(got, want40) and not np.array_equal(want40, want)

    # the same frame from two device scenes, 8 rows each
    both, k = host.MultiRenderer([0, 0], block_rows=8).render(om, W, H, light)
    assert k == n and np.array_equal(both, want)
