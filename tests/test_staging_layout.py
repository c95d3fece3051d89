"""The layout of a *_host call's device mirrors (learnraytracing_amd/csrc/lrt_staging.h).

The header is plain C++, so a stand-alone program that includes nothing else of the library is
compiled with the address and undefined-behaviour sanitizers and run: no GPU, no library load.
It walks every list of up to six buffers whose items are an RGBA plane (16 B per pixel) or a word
plane (4 B per pixel), each absent, read, written or updated in place, at 1, 3 and 67 x 45 pixels
(the 12 B and 12,060 B word planes are no multiple of 16: the rounding is exercised), and checks
what HostMirrors relies on.
"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "learnraytracing_amd", "csrc")

PROGRAM = r"""
#include "lrt_staging.h"

#include <cstdio>
#include <cstdlib>

using lrt::StagingPlan;

#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            std::fprintf(stderr, "line %d: %s\n", __LINE__, #c);        \
            std::exit(1);                                               \
        }                                                               \
    } while (0)

static char host[StagingPlan::kCapacity + 1];   // addresses only: nothing is read through them

// item i of a list: its plane (0: 16 B per pixel, 1: 4 B) and how it is used
enum Use { kAbsent, kIn, kOut, kInPlace, kUses };

static long check_lists(size_t px) {
    const size_t plane[2] = {16 * px, 4 * px};
    long lists = 0;
    for (int n = 0; n <= 6; ++n) {
        int codes = 1;
        for (int i = 0; i < n; ++i) codes *= 2 * kUses;
        for (int code = 0; code < codes; ++code) {
            StagingPlan p;
            int use[6];
            size_t size[6], want_total = 0;
            for (int i = 0, c = code; i < n; ++i, c /= 2 * kUses) {
                use[i] = c % kUses;
                size[i] = plane[c / kUses % 2];
                const void* in = use[i] == kIn || use[i] == kInPlace ? &host[i] : nullptr;
                void* out = use[i] == kOut || use[i] == kInPlace ? &host[i] : nullptr;
                CHECK(p.add(in, out, size[i]) == i);
                if (use[i] != kAbsent) want_total += (size[i] + 15) / 16 * 16;
            }
            CHECK(p.count == n);
            // total() is the sum of the rounded sizes: an absent item takes no space, an item in place one range
            CHECK(p.total() == want_total);
            for (int i = 0; i < n; ++i) {
                CHECK(p.present(i) == (use[i] != kAbsent));
                if (!p.present(i)) continue;
                CHECK(p.offset(i) % 16 == 0);
                CHECK(p.item[i].bytes == size[i]);
                CHECK(p.offset(i) + size[i] <= p.total());
                for (int j = 0; j < i; ++j)
                    if (p.present(j))
                        CHECK(p.offset(j) + size[j] <= p.offset(i) || p.offset(i) + size[i] <= p.offset(j));
            }
            ++lists;
        }
    }
    return lists;
}

int main() {
    long lists = 0;
    const size_t pixels[3] = {1, 3, 67 * 45};
    for (size_t px : pixels) lists += check_lists(px);
    // past the capacity nothing is added
    StagingPlan p;
    for (int i = 0; i < StagingPlan::kCapacity; ++i) CHECK(p.add(&host[i], nullptr, 12) == i);
    const size_t total = p.total();
    CHECK(total == 16 * (size_t)StagingPlan::kCapacity);
    CHECK(p.add(&host[StagingPlan::kCapacity], nullptr, 12) == -1);
    CHECK(p.add(nullptr, nullptr, 12) == -1);
    CHECK(p.count == StagingPlan::kCapacity && p.total() == total);
    std::printf("ok %ld lists\n", lists);
    return 0;
}
"""


def test_staging_layout(tmp_path):
    src = tmp_path / "staging_layout.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "staging_layout"
    # (the sanitizers' runtimes linked into the program: it runs whatever else the loader brings in)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-O1", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-I" + CSRC, "-o", str(exe),
                    str(src)], check=True)
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    # 3 pixel counts x sum over n = 0 .. 6 of 8^n lists
    assert p.stdout.strip() == "ok %d lists" % (3 * sum(8 ** n for n in range(7)))
