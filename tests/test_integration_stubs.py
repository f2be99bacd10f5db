"""INTEGRATION.md's reference-side stubs go through a compiler: `HipHashBuild.hpp` (with ENABLE_PROBE 0 and 1, as the
reference's config.h switches it) is compiled AND linked against libhtmjoin_hip.so, and `HIP_PRO` is compiled against
the reference's own mc/src/types.h + prj_params.h, as build() left them in oracle/_ref/include (oracle/Makefile; skipped
where build() had no reference checkout to take them from, e.g. on the GPU box). No GPU needed: nothing is run beyond a call that fails with HJ_ERR_NO_DEVICE here."""
import os
import re
import subprocess

import pytest

from htm_hashjoin_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_INCLUDE = os.path.join(ROOT, "oracle", "_ref", "include")    # build products, never committed


def _blocks(lang):
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    return re.findall(r"```" + lang + r"\n(.*?)```", text, flags=re.S)


@pytest.mark.parametrize("enable_probe", [0, 1])
def test_hiphashbuild_stub_compiles_and_links(tmp_path, enable_probe):
    stub = next(b for b in _blocks("cpp") if "inline void HipHashBuild" in b)
    (tmp_path / "HipHashBuild.hpp").write_text(stub)
    (tmp_path / "config.h").write_text(f"#define ENABLE_PROBE {enable_probe}\n")        # what the reference's config.h:4 sets
    call = ("HipHashBuild(r, 4, r, 4, 2, 64, 4);" if enable_probe else "HipHashBuild(r, 4, 2, 64, 4);")
    (tmp_path / "use.cpp").write_text(
        '#include <cstdint>\n#include <cstdlib>\n#include "HipHashBuild.hpp"\n'
        "int main(int argc, char**) { uint64_t r[4] = {1, 2, 3, 4}; if (argc > 100) { " + call + " } return 0; }\n")
    exe = tmp_path / "use"
    cmd = ["g++", "-std=c++14", "-Wall", "-Werror", "-I", str(tmp_path), "-I", os.path.join(ROOT, "include"),
           str(tmp_path / "use.cpp"), "-o", str(exe), "-L", os.path.dirname(_lib.LIB_PATH), "-lhtmjoin_hip",
           "-Wl,-rpath," + os.path.dirname(_lib.LIB_PATH)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert subprocess.run([str(exe)]).returncode == 0


def test_main_cpp_dispatch_line_names_the_stub():
    assert any('cmdParams.algo == "hip"' in b and "HipHashBuild(" in b for b in _blocks("cpp"))


@pytest.mark.skipif(not os.path.isfile(os.path.join(REF_INCLUDE, "types.h")),
                    reason="oracle/_ref/include not built (build() had no reference checkout)")
def test_hip_pro_stub_compiles_against_the_references_types(tmp_path):
    stub = next(b for b in _blocks("c") if "HIP_PRO" in b)
    # relation_t / tuple_t come from the reference's own headers (oracle/_ref/include: build products, never committed)
    (tmp_path / "hip_pro.c").write_text('#include <stdint.h>\n#include "types.h"\n#include "prj_params.h"\n' + stub)
    cmd = ["gcc", "-std=gnu99", "-Wall", "-Werror", "-fsyntax-only", "-DHAVE_CONFIG_H", "-I", REF_INCLUDE,
           "-I", os.path.join(ROOT, "include"), str(tmp_path / "hip_pro.c")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
