"""The cache policy of the device memory pool and of the pinned result cache (analiticcl_amd/csrc/block_cache.hpp: no HIP, no lock
of its own) driven by tests/block_cache/main.cpp with a counting fake allocator, under both parameter sets of runtime.hip: best fit
within the slack and not a byte beyond, oldest block out first, evicted blocks released by the next miss / a drain / beyond the
deferred bound and never by the give-back that evicted them, blocks above the limit and unpinned ones never cached, unknown pointers
reported, nothing live after a drain -- under ASan + UBSan (no leak, no double free), and four threads through one mutex-guarded owner
under TSan."""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp_path, name, sanitize):
    exe = tmp_path / name
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Werror", *sanitize, "-pthread",
           "-I", os.path.join(REPO, "analiticcl_amd", "csrc"), "-o", str(exe), os.path.join(REPO, "tests", "block_cache", "main.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return str(exe)


def test_block_cache_policy_under_asan_ubsan(tmp_path):
    exe = _build(tmp_path, "block_cache_asan", ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, "policy"], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.strip() == "OK policy"


def test_block_cache_threads_under_tsan(tmp_path):
    exe = _build(tmp_path, "block_cache_tsan", ["-fsanitize=thread"])
    env = dict(os.environ, TSAN_OPTIONS="halt_on_error=1:second_deadlock_stack=1")
    r = subprocess.run([exe, "threads"], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0 and "WARNING: ThreadSanitizer" not in r.stderr, (r.stdout[-2000:], r.stderr[-6000:])
    assert r.stdout.strip() == "OK threads"
