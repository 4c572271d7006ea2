"""Write tests/golden/mcmc_oracle64.npz: the float64 oracle's results for the teacher-forced MALA iterations and the free-running ULA chains of
tests/test_gpu_mcmc.py (minutes of CPU, hence a fixture), with the float32 oracle's distances from them, from which the tests' bars are
derived.  The oracle and the inputs are the test file's own (``write_goldens`` there); nothing here needs a GPU or the reference.

    python -m ramp_amd.tools.make_mcmc_goldens [energy] [mala] [comp] [ula]      (no argument: everything; ula-ddim: the DDIM chain only)
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

if __name__ == "__main__":
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import test_gpu_mcmc
    test_gpu_mcmc.write_goldens(**({'parts': tuple(sys.argv[1:])} if sys.argv[1:] else {}))
