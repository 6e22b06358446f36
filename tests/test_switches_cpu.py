"""No environment variable picks a kernel family: the Winograd and chain-kernel A/B variables of earlier rounds are gone from the
Python modules and from the library (the tests flip module attributes with monkeypatch instead)."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RETIRED = {'T2O_WINOGRAD': '0', 'T2O_WINOGRAD_FUSED': '0', 'T2O_WINOGRAD_WGRAD': '0', 'T2O_WINOGRAD_MIN_C': '128',
           'T2O_WINO_GEMM': 'lib', 'T2O_CHAIN_STATIC': '0'}


def test_retired_variables_change_no_module_switch():
    code = ("import sys\n"
            "sys.path.insert(0, %r)\n"
            "import t2onet_amd.encoder as E\n"
            "import t2onet_amd.functional as T\n"
            "assert E._WINOGRAD is True and E._WINO_FUSED is True and E._WINO_WGRAD is True, (E._WINOGRAD, E._WINO_FUSED, E._WINO_WGRAD)\n"
            "assert E._WINO_MIN_C == 256, E._WINO_MIN_C\n"
            "assert not hasattr(T, '_OWN_WINO_GEMM') and not hasattr(T, '_CONV_OWN')\n"
            "print('constant')\n" % ROOT)
    r = subprocess.run([sys.executable, '-c', code], env=dict(os.environ, **RETIRED), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().splitlines()[-1:] == ['constant'], r.stdout + r.stderr


def test_library_reads_no_chain_variable():
    from t2onet_amd import build
    with open(build.build(), 'rb') as f:
        assert b'T2O_CHAIN_STATIC' not in f.read()
