"""The bags a wavefront of a trained pooled kernel owns (hip_pooled.h: pooledBagsPerWave, which launchPooled and
launchPooledUnion share), without a GPU: a g++ program that includes the header alone prints the rule over a grid, and the
grid is compared with the formula as the two launch functions each spelled it before they shared it, restated here."""
import itertools
import os
import subprocess

from conftest import REPO

CSRC = os.path.join(REPO, 'memb_amd', 'csrc')

PROGRAM = r'''
#include "hip_pooled.h"

#include <cstdio>

int main()
{
    unsigned long long tilesSwitch, wordsPerWave, n, bags, cuCount, wavesPerCu;
    while (std::scanf("%llu %llu %llu %llu %llu %llu", &tilesSwitch, &wordsPerWave, &n, &bags, &cuCount, &wavesPerCu) == 6) {
        std::printf("%u\n", memb_pooled::pooledBagsPerWave(
            tilesSwitch, static_cast<uint32_t>(wordsPerWave), n, bags, static_cast<uint32_t>(cuCount),
            static_cast<uint32_t>(wavesPerCu)));
    }
    return 0;
}
'''

POOLED_TILES_PER_WAVE = 4


def bags_per_wave(tiles_switch, words_per_wave, n, bags, cu_count, waves_per_cu):
    """launchPooled's five lines: about tiles_per_wave tiles of entries per wavefront, fewer while the grid would not fill
    the CUs, at most 1 << 16 bags"""
    tiles_per_wave = tiles_switch if tiles_switch else POOLED_TILES_PER_WAVE
    entries_per_bag = max(1, n // max(bags, 1))
    fills_the_cus = max(1, bags // (cu_count * waves_per_cu))
    return min(min(max(1, tiles_per_wave * words_per_wave // entries_per_bag), fills_the_cus), 1 << 16)


def grid():
    cases = list(itertools.product(
        (0, 1, 9),                                             # the tiles_per_wave switch: unset, and two settings
        (1, 16, 64),                                           # words per wavefront: 64, 4 and 1 lanes per word
        (0, 5, 100000, 1 << 22, (1 << 37)),                    # entries
        (1, 2, 100000, 7167, 7168, 7169, 25000, 1 << 22, (1 << 37) - 1),   # bags
        ((256, 28), (1, 1))))                                  # CUs x wavefronts per CU (MI355X; a grid one bag fills)
    cases = [(switch, words, n, bags, cus, waves) for switch, words, n, bags, (cus, waves) in cases]
    named = {
        'no entries': (0, 16, 0, 100000, 256, 28),
        'fewer entries than bags': (0, 16, 5, 100000, 256, 28),
        'one bag holds every entry': (0, 16, 100000, 1, 256, 28),
        'switch set': (9, 16, 1 << 22, 1 << 22, 256, 28),
        'filling the CUs binds': (0, 16, 100000, 25000, 256, 28),
        'the tile budget binds': (0, 16, 1 << 22, 1 << 20, 256, 28),
        'clamped': (1 << 20, 16, 1 << 20, 1 << 20, 1, 1),
        'clamped on an MI355X': (5000, 16, 1 << 30, 1 << 30, 256, 28),
    }
    return cases + list(named.values()), named


def test_the_grid_reaches_every_term_of_the_rule():
    # (of the restated formula: what each named case is there for)
    _, named = grid()
    assert bags_per_wave(*named['no entries']) == 13 and bags_per_wave(*named['fewer entries than bags']) == 13
    assert bags_per_wave(*named['one bag holds every entry']) == 1
    assert bags_per_wave(*named['switch set']) == 9 * 16 != bags_per_wave(0, *named['switch set'][1:]) == 4 * 16
    assert bags_per_wave(*named['filling the CUs binds']) == 25000 // (256 * 28) == 3 < 4 * 16 // 4
    assert bags_per_wave(*named['the tile budget binds']) == 4 * 16 // 4 == 16 < (1 << 20) // (256 * 28)
    assert bags_per_wave(*named['clamped']) == 1 << 16 and bags_per_wave(*named['clamped on an MI355X']) == 1 << 16


def test_bags_per_wave_is_the_rule_of_both_launch_functions(tmp_path):
    source, binary = str(tmp_path / 'bags_per_wave.cpp'), str(tmp_path / 'bags_per_wave')
    with open(source, 'w') as f:
        f.write(PROGRAM)
    # (the header alone, by plain g++: no HIP, no other header of the project)
    build = subprocess.run(['g++', '-std=c++17', '-Wall', '-Wextra', '-Werror', '-I', CSRC, source, '-o', binary],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout
    cases, _ = grid()
    run = subprocess.run([binary], input=''.join('{} {} {} {} {} {}\n'.format(*case) for case in cases),
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
    assert run.returncode == 0, run.stdout
    got = [int(line) for line in run.stdout.split()]
    assert len(got) == len(cases)
    for case, value in zip(cases, got):
        assert value == bags_per_wave(*case), case
