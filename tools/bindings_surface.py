"""The Python-visible surface of the native extension `_memb`, as text.

One line per callable of the module and of its classes Reader, Builder and WordBatch, with the docstring pybind11
generates for it (the signature block: positional order, keyword names, defaults, return type, and the doc text), and
one line per module attribute with its value; sorted. Dunder names are left out, except each class's `__init__`: the
order in which its overloads were registered shows there and nowhere else.

    python tools/bindings_surface.py            prints the text
    python tools/bindings_surface.py FILE       writes it to FILE

tests/test_bindings_surface.py compares this text with tests/golden/bindings_surface.txt, so a change to the binding
sources that moves a name, an argument or a default is seen without a GPU.
"""
import json
import os
import sys

CLASSES = ('Builder', 'Reader', 'WordBatch')


def _dunder(name):
    return name.startswith('__') and name.endswith('__')


def surface_text(module):
    lines = []
    for name in dir(module):
        if _dunder(name):
            continue
        value = getattr(module, name)
        if name in CLASSES:
            for member in dir(value):
                if _dunder(member) and member != '__init__':
                    continue
                lines.append('{}.{} {}'.format(name, member, json.dumps(getattr(value, member).__doc__)))
        elif callable(value):
            lines.append('{} {}'.format(name, json.dumps(value.__doc__)))
        else:
            lines.append('{} = {!r}'.format(name, value))
    return '\n'.join(sorted(lines)) + '\n'


if __name__ == '__main__':
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from memb_amd import _memb
    text = surface_text(_memb)
    if len(sys.argv) > 1:
        with open(sys.argv[1], 'w') as output:
            output.write(text)
    else:
        sys.stdout.write(text)
