"""CPU: what the blocked fit decides before its first launch (csrc/fit_plan.hpp, plan_fit), through a stand-alone program
(tests/fit_plan_driver.cpp, built with g++ under AddressSanitizer + UBSan where this g++ has them; nothing loaded into
python, nothing near a GPU), against the rule restated here from the header's comments:

* the outer block: all of Np up to 1024, 256 up to 1280, 1024 from 6144, else 512; TGP_OB overrides; a last, partial
  outer block whose length is not a power of two (1024 can leave 768) forces 512;
* the inverse runs behind the panel chain when there is more than one outer block and Np <= 9216;
* an outer block's panels are fused when its first update has at most TGP_PANEL_FUSE_TILES tiles."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = list(range(256, 12288 + 1, 256))
SWITCHES = ["TGP_OB", "TGP_BGINV", "TGP_BGINV_MAX", "TGP_PANEL", "TGP_PANEL_LA", "TGP_PANEL_FUSE", "TGP_PANEL_FUSE_TILES"]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("fit_plan")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    probe = tmp / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run(["g++"] + san + [str(probe), "-o", str(tmp / "probe")], capture_output=True, timeout=300).returncode != 0:
        san = []                                   # (no sanitizer runtime here: the same program without it)
    exe = str(tmp / "fit_plan")
    built = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall"] + san + ["-I" + os.path.join(ROOT, "turbo_amd", "csrc"),
                            os.path.join(ROOT, "tests", "fit_plan_driver.cpp"), "-o", exe], capture_output=True, text=True, timeout=300)
    assert built.returncode == 0, built.stderr[-3000:]

    def run(*args, **env):
        e = {k: v for k, v in os.environ.items() if k not in SWITCHES}
        e.update(env)
        out = subprocess.run([exe, *args], env=e, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0 and "runtime error" not in out.stderr and "ERROR" not in out.stderr, out.stdout[-500:] + out.stderr[-3000:]
        return [ln.split() for ln in out.stdout.splitlines()]
    return run


def expected(Np, ob_env):
    """(OB, nblk, tail, inverse behind the chain) by the rule of the comments"""
    if ob_env:
        OB = ob_env
    elif Np <= 1024:
        OB = Np
    elif Np <= 1280:
        OB = 256
    elif Np >= 6144:
        OB = 1024
    else:
        OB = 512
    tail = Np % OB
    if bin(tail).count("1") > 1:        # not a power of two (0 = no partial block)
        OB = 512
    return OB, -(-Np // OB), Np % OB, int(Np > OB and Np <= 9216)


@pytest.mark.parametrize("ob_env", [None, 256, 512, 1024], ids=["unset", "ob256", "ob512", "ob1024"])
def test_outer_block_over_every_size(driver, ob_env):
    rows = driver("sizes", **({"TGP_OB": str(ob_env)} if ob_env else {}))
    got = {int(r[0]): tuple(int(v) for v in r[1:]) for r in rows}
    assert sorted(got) == SIZES
    for Np in SIZES:
        assert got[Np] == expected(Np, ob_env), (Np, ob_env, got[Np], expected(Np, ob_env))
        assert got[Np][2] != 768, (Np, ob_env, got[Np])
    if ob_env == 1024:
        assert got[1792][0] == 512
    if ob_env is None:
        assert [got[Np][0] for Np in (6912, 7936, 8960)] == [512, 512, 512]
        assert got[6144][0] == 1024 and got[8192][0] == 1024 and got[1280][0] == 256 and got[1024] == (1024, 1, 0, 0)


def test_inverse_eligibility_follows_its_switches(driver):
    assert all(r[4] == "0" for r in driver("sizes", TGP_BGINV="0"))
    got = {int(r[0]): int(r[4]) for r in driver("sizes", TGP_BGINV_MAX="2048")}
    assert [Np for Np in SIZES if got[Np]] == [1280, 1536, 1792, 2048]


def test_panel_mode_is_decided_per_outer_block(driver):
    rows = driver("panels", "1100", "1280", TGP_OB="256", TGP_PANEL_FUSE_TILES="20")
    assert rows == [["0", "51", "pivot_beside"], ["256", "39", "pivot_beside"], ["512", "27", "pivot_beside"],
                    ["768", "15", "fused"], ["1024", "1", "fused"]]
    # the defaults fuse all five; without the look-ahead, or with another diagonal variant, none
    assert [r[2] for r in driver("panels", "1100", "1280", TGP_OB="256")] == ["fused"] * 5
    assert [r[2] for r in driver("panels", "1100", "1280", TGP_OB="256", TGP_PANEL_FUSE="0")] == ["pivot_beside"] * 5
    assert [r[2] for r in driver("panels", "1100", "1280", TGP_OB="256", TGP_PANEL_LA="0")] == ["plain5"] * 5
    assert [r[2] for r in driver("panels", "1100", "1280", TGP_OB="256", TGP_PANEL="3")] == ["plain3"] * 5
    # N = 129: Nr = 192 of Np = 256, one outer block of three real panels
    assert driver("panels", "129", "256") == [["0", "4", "fused"]]
