#!/usr/bin/env python3
"""Writes the fixtures of the reference package that the CPU tests read, so that the suite needs no reference checkout:

  tests/golden/reference_tasks/*.yaml   the package's shipped task files (config/tasks/), verbatim
  tests/golden/reference_package.json   what tests/test_integration_recipe.py checks the INTEGRATION.md recipe against:
                                        the targets and directory-wide include paths of its CMakeLists.txt, the names of
                                        its headers, messages and services, and the <bimanual_planning_ros/...> include
                                        lines of every source and header (file names only, no code)

usage: python tests/golden/make_reference_package.py <reference checkout>"""
import glob
import json
import os
import re
import shutil
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
INCLUDE = re.compile(r'#include\s*[<"](bimanual_planning_ros/[\w.]+)[>"]')


def cmake_commands(text):
    """[(command, [arguments])] of a CMake file (comments stripped; no nested parentheses in this package)"""
    text = re.sub(r"#[^\n]*", "", text)
    return [(m.group(1).lower(), m.group(2).split()) for m in re.finditer(r"(\w+)\s*\(([^()]*)\)", text)]


def main(checkout):
    pkg = os.path.join(checkout, "src", "bimanual_planning_ros")
    tasks = sorted(glob.glob(os.path.join(pkg, "config", "tasks", "*.yaml")))
    out_tasks = os.path.join(HERE, "reference_tasks")
    os.makedirs(out_tasks, exist_ok=True)
    for f in tasks:
        shutil.copyfile(f, os.path.join(out_tasks, os.path.basename(f)))
    cmake = [[c, a] for c, a in cmake_commands(open(os.path.join(pkg, "CMakeLists.txt")).read())
             if c in ("add_library", "add_executable", "include_directories")]
    inc_dir = os.path.join(pkg, "include", "bimanual_planning_ros")
    files = sorted(["include/bimanual_planning_ros/" + h for h in os.listdir(inc_dir)] +
                   [os.path.relpath(f, pkg) for f in glob.glob(os.path.join(pkg, "src", "*.cpp"))])
    includes = {f: INCLUDE.findall(open(os.path.join(pkg, f)).read()) for f in files}
    stems = lambda d: sorted(os.path.splitext(f)[0] for f in os.listdir(os.path.join(pkg, d)))
    fixture = {"cmake_commands": cmake, "headers": sorted(os.listdir(inc_dir)), "messages": stems("msg"),
               "services": stems("srv"), "includes": includes}
    with open(os.path.join(HERE, "reference_package.json"), "w") as fh:
        json.dump(fixture, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("%d task files, %d CMake commands, %d files' includes" % (len(tasks), len(cmake), len(includes)))


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
