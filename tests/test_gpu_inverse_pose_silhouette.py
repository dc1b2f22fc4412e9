"""examples/inverse_pose.py --silhouette: pose recovery on the view that contains the silhouette of the whole field, the
primary rays reparameterised (reparameterize_ray -> hf_reparam_backward_full for to_world), the samples splatted at the
film position of the reparameterised ray.  The bounds are those of test_inverse_pose_recovers_translation_and_yaw
(test_gpu_transform_scenes.py) for the same start and target pose."""
import math
import os
import sys

import pytest

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))


def test_inverse_pose_silhouette_recovers_translation_and_yaw(monkeypatch):
    import torch
    import inverse_pose as ip
    from hf_amd import shape as sh
    assert torch.cuda.is_available()

    def boom(*a, **k):
        raise AssertionError("the per-sample path was taken")
    monkeypatch.setattr(sh, "_reparam_backward_per_sample", boom)      # to_world's gradient: the fused kernel
    target, start, final, losses = ip.recover_silhouette(steps=150)
    err0 = max(abs(start[0] - target[0]), abs(start[1] - target[1]))
    err = max(abs(final[0] - target[0]), abs(final[1] - target[1]))
    yaw_err = abs(final[2] - target[2])
    print(f"pose: start {start}, recovered {final}, loss {losses[0]:.3e} -> {losses[-1]:.3e}")
    assert losses[-1] < 1e-3 * losses[0], (losses[0], losses[-1])
    assert err < 5e-4 and err < 0.01 * err0, (final, target)          # translation, object units (a cell: 7.8e-3)
    assert yaw_err < math.radians(0.02), (math.degrees(yaw_err), final)


def test_the_film_position_follows_the_direction():
    """film_position inverts pinhole(): the splat position of a reparameterised ray is that of its direction"""
    import torch
    import inverse_pose as ip
    ray, pos = ip.pinhole(64, 4, "cuda", 1.3)
    assert float((ip.film_position(ray.d, 64, 1.3) - pos).abs().max()) < 1e-3      # pixels
    # the splat of a constant is that constant wherever a pixel received weight
    img = ip.splat(torch.full_like(pos[0], 0.7), torch.ones_like(pos[0]), pos, 64)
    assert torch.allclose(img, torch.full_like(img, 0.7), atol=1e-6)
