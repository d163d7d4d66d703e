"""CPU side of the C++ multi-GPU merge path: eds2leds's --gpus option, which is checked before any file or device is
touched."""
import os
import subprocess


def _eds2leds():
    from test_host_cpp import BUILD, _build_host
    _build_host()
    return os.path.join(BUILD, "eds2leds")


def test_eds2leds_help_lists_gpus():
    r = subprocess.run([_eds2leds(), "--help"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0
    assert "--gpus" in r.stdout


def test_eds2leds_gpus_out_of_range(tmp_path):
    # the files do not exist and no device is visible: the option is refused before either is looked at
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1")
    for bad in ("0", "65"):
        r = subprocess.run([_eds2leds(), "-i", str(tmp_path / "none.eds"), "-s", str(tmp_path / "none.seds"), "-l", "4",
                            "--gpus", bad], capture_output=True, text=True, timeout=120, env=env)
        assert r.returncode == 1
        assert "--gpus must be between 1 and 64" in r.stderr
        assert "not found" not in r.stderr and "Cannot open" not in r.stderr
        assert not (tmp_path / "none_l4.leds").exists() and not (tmp_path / "none_l4.seds").exists()
        assert os.listdir(tmp_path) == []
