"""The module-level drop-in: the reference's menu script, unchanged, must import the ENGINE's six modules
and reach the engine's runners when started through dropin/run_app.py -- and plain `python Scripts/app.py` must be known NOT to.
The menu script is tests/menu_like.py (the same contract as the reference's Scripts/app.py), set up as <tmp>/Scripts/app.py beside six
same-named decoy modules that stand for the reference's own Keras modules and fail at import: the launcher must reach past them."""
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
DROPIN = os.path.join(ROOT, "one-stop-for-covid-19-infection-and-lung-segmentation-plus-classification_amd", "dropin")
MODULES = ("task1_crossval_3folds_unet", "task1_crossval_4folds_unet", "task1_preprocessing_plus_unet_with_comments", "task1_unet_plus_plus",
           "task2_covid19_classifcation", "task3_lung_segmentation_unet")
DECOY = "decoy sibling module imported"


def make_app(tmp_path):
    """<tmp>/Scripts/app.py (the menu stand-in) + the six task modules next to it, each raising at import"""
    d = tmp_path / "Scripts"
    d.mkdir()
    (d / "app.py").write_text(open(os.path.join(HERE, "menu_like.py")).read())
    for m in MODULES:
        (d / f"{m}.py").write_text(f"raise ImportError({DECOY!r} + ': {m}')\n")
    return str(d / "app.py")


def run_app(app, word, extra_env=None, timeout=600):
    env = dict(os.environ, UNET_DROPIN_TRACE="1", **(extra_env or {}))
    env.pop("PYTHONPATH", None)
    return subprocess.run([sys.executable, os.path.join(DROPIN, "run_app.py"), app], input=word + "\n", capture_output=True, text=True, env=env, timeout=timeout)


def assert_dropins_imported(out):
    lines = [l for l in out.splitlines() if l.startswith("[dropin] ")]
    assert len(lines) == 6, out
    for l in lines:
        assert os.path.dirname(l.split(" <- ")[1]) == DROPIN, l


def test_reference_app_text_resolves_the_dropins_and_exits_cleanly_on_an_unknown_choice(tmp_path):
    r = run_app(make_app(tmp_path), "seven")              # APP:29 advertises 'seven'; no branch takes it -> the script just ends
    assert r.returncode == 0, r.stderr[-2000:]
    assert "Enter one of" in r.stdout                     # the menu script's own prompt was executed
    assert DECOY not in r.stderr
    assert_dropins_imported(r.stdout)


def test_reference_app_three_reaches_the_engine_and_fails_loudly_without_a_gpu(tmp_path):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present: covered by the -m gpu test below")
    r = run_app(make_app(tmp_path), "three", {"UNET_EPOCHS": "1", "UNET_SAMPLES": "8", "UNET_SIZE": "32"})
    assert r.returncode != 0 and "UNetHipError" in r.stderr, (r.returncode, r.stderr[-2000:])       # no CPU fallback: the HIP engine refuses loudly
    assert DECOY not in r.stderr                          # (what a sibling of the script dies with when it is imported instead)
    assert_dropins_imported(r.stdout)


def test_menu_stand_in_resolves_the_dropins():
    r = run_app(os.path.join(HERE, "menu_like.py"), "seven")
    assert r.returncode == 0, r.stderr[-2000:]
    assert_dropins_imported(r.stdout)


@pytest.mark.gpu
@pytest.mark.parametrize("word,needle", [("three", "test loss, test dice coefficient:"), ("six", "test loss, test dice coefficient:")])
def test_menu_choice_runs_on_the_engine(word, needle, tmp_path):
    """APP:44-45 / 56-57 through the launcher on the MI355X: 'three' (infection hold-out) and 'six' (lung) complete and print the reference's
    summary lines."""
    app = make_app(tmp_path)
    env = {"UNET_EPOCHS": "1", "UNET_SAMPLES": "8", "UNET_SIZE": "32"}
    p = subprocess.run([sys.executable, os.path.join(DROPIN, "run_app.py"), app], input=word + "\n", capture_output=True, text=True,
                       env=dict(os.environ, UNET_DROPIN_TRACE="1", **env), timeout=900, cwd=str(tmp_path))
    assert p.returncode == 0, p.stderr[-3000:]
    assert needle in p.stdout and "Best dice score:" in p.stdout and "Best Threshold for Recall:" in p.stdout
    assert_dropins_imported(p.stdout)
    assert os.path.exists(tmp_path / "unet_covid_weights_dice_coeff.hdf5")          # T1:1044 checkpoint written where the reference writes it (cwd)
