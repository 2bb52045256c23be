"""Host-only: rt_sample_units, the launcher's restatement of the sample kernels' live_take (csrc/pt_sample.hpp), against
a Python restatement of that device function.  For every capacity, pixels per unit and pair of raw counters — counters
past the capacity included, which the kernels clamp — every unit below the returned number takes at least one pixel,
every unit from it on takes none, and the takes add up to the clamped counts."""
import pytest

import cases

rt = cases.rt


def live_take(cap, count_light, count_heavy, unit, want):
    """→ (first entry, entries) of `unit`: live_take of csrc/pt_sample.hpp, line by line."""
    cnt_l = min(count_light, cap)
    cnt_h = min(count_heavy, cap - cnt_l)
    units_h = (cnt_h + want - 1) // want if want else 0
    heavy = unit < units_h
    cnt = cnt_h if heavy else cnt_l
    start = min((unit if heavy else unit - units_h) * want, cnt)
    first = (cap - cnt_h if heavy else 0) + start
    return first, min(want, cnt - start)


@pytest.mark.parametrize("cap", range(0, 65, 8))
def test_units_cover_exactly_the_live_list(built, cap):
    for ppw in range(1, 17):
        for light in range(0, cap + 4):
            for heavy in range(0, cap + 4):
                units = rt.sample_units(cap, ppw, light, heavy)
                cnt_l = min(light, cap)
                cnt_h = min(heavy, cap - cnt_l)
                takes = [live_take(cap, light, heavy, u, ppw) for u in range(units + 3)]
                key = (cap, ppw, light, heavy, units)
                assert all(n >= 1 for _, n in takes[:units]), key
                assert all(n == 0 for _, n in takes[units:]), key
                assert sum(n for _, n in takes) == cnt_l + cnt_h, key
                # (and the parts lie where the kernels look for them: heavy from the end downwards, light from 0)
                assert all(0 <= f and f + n <= cap for f, n in takes), key
                assert units <= -(-cap // ppw) + 1, key     # never more than the worst-case grid


def test_refuses_what_it_cannot_divide(built):
    with pytest.raises(rt.RtError):
        rt.sample_units(64, 0, 1, 1)
    assert rt.sample_units(0, 4, 7, 7) == 0
    assert rt.sample_units(2 ** 32 - 256, 1, 2 ** 32 - 1, 2 ** 32 - 1) == 2 ** 32 - 256
