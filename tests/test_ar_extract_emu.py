"""mrz_ar_extract / mrz_ar_extract_mrz on the wave64 emulator: tests/_ar_extract_checks.py."""
import pytest

import modern_rzip_amd as m
from tests import _ar_extract_checks as X

EMU = True


@pytest.fixture(scope="module")
def lib(emu_lib):
    return emu_lib


@pytest.fixture(scope="module")
def ctx(lib):
    with m.RzipContext(lib=lib) as c:
        yield c


def test_abi_unchanged(lib):
    X.check_abi(lib)


@pytest.mark.parametrize("where,out_where", [("host", "host"), ("device", "device"), ("host", "device"), ("device", "host")])
@pytest.mark.parametrize("which_archive", ["created", "ref"])
def test_extract(ctx, which_archive, where, out_where):
    X.check_extract(ctx, EMU, which_archive, where, out_where)


@pytest.mark.parametrize("where", ["host", "device"])
def test_verify_names_the_members(ctx, where):
    X.check_verify(ctx, EMU, where)


def test_corrupt_archives_and_arguments(ctx):
    X.check_corrupt_and_arguments(ctx, EMU)


@pytest.mark.parametrize("out_where", ["host", "device"])
@pytest.mark.parametrize("kind", ["n", "l"])
def test_extract_from_mrz(ctx, kind, out_where):
    X.check_extract_mrz(ctx, EMU, kind, out_where)


@pytest.mark.parametrize("kind", ["n", "l"])
def test_one_small_member_uploads_little(ctx, kind):
    X.check_one_small_member(ctx, kind)


@pytest.mark.parametrize("kind", ["n", "l"])
def test_mrz_verify_and_corrupt(ctx, kind):
    X.check_mrz_verify_and_corrupt(ctx, kind)


def test_c99_caller_program(lib, tmp_path):
    """tests/c/capi_extract_test.c: a plain C99 program linked against the emulator build drives the four new entry
    points"""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "capi_extract_test")
    subprocess.run(["gcc", "-std=c99", "-O1", "-I" + os.path.join(root, "include"),
                    os.path.join(root, "tests", "c", "capi_extract_test.c"), "-o", exe,
                    "-L" + os.path.join(root, "tests", "emu"), "-l:libmrzgpu_emu.so"], check=True)
    env = dict(os.environ, LD_LIBRARY_PATH=os.pathsep.join([os.path.join(root, "tests", "emu"),
                                                            os.environ.get("LD_LIBRARY_PATH", "")]))
    out = subprocess.run([exe], check=True, env=env, stdout=subprocess.PIPE, text=True, timeout=120).stdout
    assert "capi_extract_test ok" in out
