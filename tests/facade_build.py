"""The headless facade library and one driver program of tests/cpp linked against it, as the GPU facade tests run them."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_driver(tmp_path, name: str, opt: str = "-O2") -> str:
    """make NO_GL=1 in melonix_amd/cpp, then tests/cpp/<name>.cpp -> tmp_path/<name>; returns the program's path."""
    lib = os.path.join(ROOT, "melonix_amd", "lib")
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "melonix_amd", "cpp"), "NO_GL=1"])
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-std=c++20", opt, "-DMELONIX_AMD_NO_GL", "-I", os.path.join(ROOT, "melonix_amd", "cpp"), "-I",
                           os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", name + ".cpp"),
                           "-o", exe, "-L", lib, "-lmelonix_facade", "-lmelonix_amd", f"-Wl,-rpath,{lib}", "-lpthread"])
    return exe
