#!/usr/bin/env python
"""Writes tests/golden/cli_flags.json: per command-line script (infer.py, eval.py,
eval_poses.py) the list of (option_strings, dest, default, type name, choices, required, help)
of every action of its build_parser(), in parser order. tests/test_cli_host.py compares the
parsers against it, so run it only on a commit whose flags are the intended ones:
    python tests/golden/make_cli_flags.py
"""
import importlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, 'cli_flags.json')
SCRIPTS = ('infer', 'eval', 'eval_poses')


def parser_flags(parser):
  """JSON-ready rows of a parser's actions; the help action (-h) included."""
  return [[list(a.option_strings), a.dest,
           None if a.default is None else a.default,
           getattr(a.type, '__name__', None), None if a.choices is None else list(a.choices),
           bool(a.required), a.help] for a in parser._actions]


def all_flags():
  if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
  return {name: parser_flags(importlib.import_module(name).build_parser()) for name in SCRIPTS}


if __name__ == '__main__':
  data = all_flags()
  with open(OUT, 'w') as f:
    json.dump(data, f, indent=1)
  print({k: len(v) for k, v in data.items()})
