"""Run one of the reference's own entry scripts on the HIP path, with zero edits to the reference checkout:

    python -m summarizer_amd.run_reference /path/to/Summarizer/summarizer/main.py -m vasnet -s tvsum -c yes --local 16

installs the module aliases (`summarizer_amd.install_as_reference`), puts the checkout on sys.path exactly like
`main.py:5` does itself, and executes the script as `__main__` with the remaining arguments (main.py:75-103 parses them).  Leading flags opt further modules in: `--sumgan-att` maps `summarizer.models.sumgan_att` to this
package, `--baselines` maps `summarizer.models.logistic` and `summarizer.models.rand` (in either order, together or alone):

    python -m summarizer_amd.run_reference --sumgan-att /path/to/Summarizer/summarizer/main.py -m sumgan_att ...
    python -m summarizer_amd.run_reference --baselines /path/to/Summarizer/benchmark.py ..."""
import os
import runpy
import sys

from . import install_as_reference


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    flags = {"--sumgan-att": ("sumgan_att",), "--baselines": ("logistic", "random")}
    opt_in = ()
    while argv and argv[0] in flags:
        opt_in += tuple(k for k in flags[argv[0]] if k not in opt_in)
        argv = argv[1:]
    if not argv or not os.path.isfile(argv[0]):
        raise SystemExit("usage: python -m summarizer_amd.run_reference [--sumgan-att] [--baselines] <reference script, e.g. "
                         "summarizer/main.py> [its arguments]")
    script = os.path.abspath(argv[0])
    sys.path.append(os.path.dirname(os.path.dirname(script)))        # the directory holding the `summarizer` package
    install_as_reference(opt_in=opt_in)
    sys.argv = [script] + argv[1:]
    runpy.run_path(script, run_name="__main__")


if __name__ == "__main__":
    main()
