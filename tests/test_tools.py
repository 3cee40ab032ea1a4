"""CPU checks of the assembly hazard scanner (tools/check_store_hazard.py): a
>8-byte vector-memory store whose data VGPRs the very next VALU instruction overwrites."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "check_store_hazard.py")

HAZARD = """_Zkernel:
	buffer_store_dwordx4 v[2:5], v14, s[24:27], s19 offen
	v_ashrrev_i32_e32 v2, 2, v13
	s_endpgm
"""
CLEAN = """_Zkernel:
	buffer_store_dwordx4 v[2:5], v14, s[24:27], s19 offen
	; sched_barrier mask(0x00000000)
	s_nop 1
	v_ashrrev_i32_e32 v2, 2, v13
	global_store_dwordx2 v[6:7], v[0:1], off
	v_lshl_add_u64 v[0:1], s[0:1], 0, v[4:5]
	s_endpgm
"""


def _run(tmp_path, text):
    f = tmp_path / "k.s"
    f.write_text(text)
    return subprocess.run([sys.executable, TOOL, str(f)], capture_output=True, text=True)


def test_store_hazard_detected(tmp_path):
    r = _run(tmp_path, HAZARD)
    assert r.returncode == 1 and "1 hazard pair(s)" in r.stdout


def test_store_hazard_clean(tmp_path):
    # a wait state in between, and an 8-byte store (not affected) followed by a write of its data
    r = _run(tmp_path, CLEAN)
    assert r.returncode == 0 and "0 hazard pair(s)" in r.stdout


def test_shipped_library_has_no_store_hazard():
    """The scanner over every gfx950 code object of the built product library (one per .hip
    translation unit), not only synthetic text."""
    import glob
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_store_hazard as H
    lib = os.path.join(ROOT, "tf_flash_attention_amd", "libfa_hip.so")
    objs = H.disassemble_library(lib)
    csrc = os.path.join(ROOT, "tf_flash_attention_amd", "csrc")

    def has_kernels(p):  # the unit's own text or a shared kernel header it includes (*_impl.h)
        text = open(p).read()
        impl = [ln.split('"')[1] for ln in text.splitlines() if ln.startswith('#include "') and '_impl.h"' in ln]
        return "__global__" in text + "".join(open(os.path.join(csrc, f)).read() for f in impl)
    # translation units with kernels (fa_api.hip has none)
    n_tu = sum(has_kernels(p) for p in glob.glob(os.path.join(csrc, "*.hip")))
    assert len(objs) == n_tu
    assert sum(d.count("buffer_store") + d.count("global_store") for _, d in objs) > 100
    found = []
    assert sum(H.scan_text(n, d, out=found.append) for n, d in objs) == 0, found


def test_setup_py_builds_through_make():
    """setup.py (the reference's setup.py / pyproject counterpart) drives the same make build."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "setup.py", "--name"], cwd=root, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().splitlines()[-1] == "tf_flash_attention_amd"
    r = subprocess.run([sys.executable, "setup.py", "--dry-run", "build_ext"], cwd=root, capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr
    assert "BuildHip: make -C" in r.stdout and "tf_flash_attention_amd" in r.stdout


# ---- tools/asm_equal.py: the SCALAR-ONLY verdict (equal counts and resources, only s_* lines moved)
ASM_EQUAL = os.path.join(ROOT, "tools", "asm_equal.py")
KERNEL_S = """	.type	_Z1kv,@function
_Z1kv:
{body}	s_endpgm
	.amdhsa_kernel _Z1kv
		.amdhsa_next_free_vgpr 2
		.amdhsa_next_free_sgpr 6
	.end_amdhsa_kernel
.Lfunc_end0:
; NumVgprs: 2
"""
LINES = ["s_load_dword s0, s[4:5], 0x0", "s_mov_b32 s1, 0", "v_mov_b32_e32 v0, s0", "v_add_u32_e32 v1, v0, v0"]


def _asm_equal(tmp_path, new_order, *flags):
    old, new = tmp_path / "old.s", tmp_path / "new.s"
    old.write_text(KERNEL_S.format(body="".join(f"\t{ln}\n" for ln in LINES)))
    new.write_text(KERNEL_S.format(body="".join(f"\t{LINES[i]}\n" for i in new_order)))
    return subprocess.run([sys.executable, ASM_EQUAL, *flags, str(old), str(new)], capture_output=True, text=True)


def test_asm_equal_scalar_only(tmp_path):
    """Two scalar lines swapped: SCALAR-ONLY, counted on its own, and accepted only under --scalar-ok."""
    r = _asm_equal(tmp_path, [1, 0, 2, 3])
    assert r.returncode == 1 and r.stdout.startswith("SCALAR-ONLY") and "1 not identical, 1 of them scalar-only" in r.stdout
    r = _asm_equal(tmp_path, [1, 0, 2, 3], "--scalar-ok")
    assert r.returncode == 0 and r.stdout.startswith("SCALAR-ONLY")
    r = _asm_equal(tmp_path, [0, 1, 2, 3])
    assert r.returncode == 0 and r.stdout.startswith("IDENTICAL") and "0 not identical" in r.stdout


def test_asm_equal_vector_line_moved(tmp_path):
    """The two vector lines swapped (counts and resources still equal): DIFFERS, whatever the flag."""
    for flags in ((), ("--scalar-ok",)):
        r = _asm_equal(tmp_path, [0, 1, 3, 2], *flags)
        assert r.returncode == 1 and r.stdout.startswith("DIFFERS") and "scalar-only" not in r.stdout
