"""Empty on purpose: the reference runs `import steerable.utils` (src/train/pyramid.py:8, src/train/train.py:8) without using it."""
