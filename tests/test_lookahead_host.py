"""CPU (no device): rt_lookahead_plan, the host function that decides how many samples the look-ahead launch of an
rt_render_again call traces (RT_OPT_LOOKAHEAD) — min(option, samples left below RT_MAX_SAMPLE, frames of W x H float4 in
the ring's budget of 1 GiB), 0 where that is below 2.  rt_render_again calls this very function."""
import pytest

import cases

rt = cases.rt
RT_MAX_SAMPLE = 65535
RT_EINVAL = -1


def test_plan_follows_option_budget_and_sample_limit(built):
    plan = rt.lookahead_plan
    assert plan(1920, 1080, 16, 0) == 16
    assert plan(3840, 2160, 16, 0) == 8            # 132.7 MB per frame: 8 of them in 1 GiB
    assert plan(16384, 16384, 16, 0) == 0          # one frame is 4 GiB
    assert plan(1920, 1080, 0, 0) == 0
    assert plan(1920, 1080, 16, RT_MAX_SAMPLE - 3) == 3
    assert plan(1920, 1080, 16, RT_MAX_SAMPLE - 1) == 0
    # every admitted option value on a small frame, and the budget's own arithmetic on a large one
    for k in range(2, 65):
        assert plan(200, 120, k, 7) == k
        assert plan(4096, 4096, k, 0) == min(k, (1 << 30) // (4096 * 4096 * 16))
    assert plan(1, 1, 64, 0) == 64
    assert rt.RayTracer.lookaheadPlan(1920, 1080, 16, 0) == 16


@pytest.mark.parametrize("args", [(1920, 1080, 1, 0), (1920, 1080, 65, 0), (1920, 1080, -1, 0), (0, 1080, 16, 0),
                                  (1920, 0, 16, 0), (-5, 7, 16, 0), (1920, -1, 0, 0)])
def test_plan_refuses_what_the_option_refuses(built, args):
    with pytest.raises(rt.RtError) as e:
        rt.lookahead_plan(*args)
    assert e.value.code == RT_EINVAL
