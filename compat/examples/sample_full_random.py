"""Reference path examples/sample_full_random.py."""
from deephisto_amd.examples.sample_full_random import main  # noqa: F401

if __name__ == "__main__":
    main()
