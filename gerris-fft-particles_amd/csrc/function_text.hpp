// function_text.hpp -- what the objects that take the text of a GfsFunction and a table of variables (the kernel of
// a GfsSourceParticulate, GfsSourceParticulateVol / ...Mass, GfsFeedParticle; boxes and trees) ask of the texts
// before anything is compiled.  Plain C++ with no HIP type, like particulate_forces.hpp: the host compiler builds it
// alone (tests/test_function_text_cpu.py).  The messages stay with the callers: a check here says which rule failed.
#pragma once
#include <cctype>
#include <cstdlib>
#include <cstring>
#include <string>

namespace gfship {

// is the text a constant (gfs_function_read: a number is kept as f->val, and needs no compilation)?  strtod takes at
// least one character and only blanks, tabs, CR or LF follow; *value = 0. otherwise
inline bool text_constant (const char * text, double * value)
{
  char * end = nullptr;
  *value = strtod (text, &end);
  while (end != text && (*end == ' ' || *end == '\t' || *end == '\n' || *end == '\r')) end++;
  if (end != text && *end == '\0') return true;
  *value = 0.;
  return false;
}

inline bool c_identifier (const char * s)
{
  if (!s || !(isalpha ((unsigned char) *s) || *s == '_')) return false;
  for (; *s; s++)
    if (!(isalnum ((unsigned char) *s) || *s == '_')) return false;
  return true;
}

// does the C text name `id' (a whole identifier, not a member and not inside a string)?
inline bool names_identifier (const std::string & e, const std::string & id)
{
  size_t p = 0;
  while (p < e.size ()) {
    if (isalpha ((unsigned char) e[p]) || e[p] == '_') {
      size_t b = p;
      while (p < e.size () && (isalnum ((unsigned char) e[p]) || e[p] == '_')) p++;
      const bool member = b > 0 && (e[b - 1] == '.' || isdigit ((unsigned char) e[b - 1]));
      if (!member && e.compare (b, p - b, id) == 0) return true;
    }
    else if (e[p] == '"') {
      p++;
      while (p < e.size () && e[p] != '"') p++;
      p++;
    }
    else
      p++;
  }
  return false;
}

// the table of variables of such an object: nvars names with nvars variables, every name a C identifier, none of
// them one of the `nbuiltin' variables of the function itself, none twice.  The first rule that fails, in the order
// of the table; q: the entry, name: the built-in name or the name that stands twice
enum TableRule { TABLE_OK = 0, TABLE_INVALID, TABLE_NO_C_NAME, TABLE_BUILTIN, TABLE_TWICE };
struct TableFault { TableRule rule; int q; const char * name; };

inline TableFault table_fault (int nvars, const char * const * names, const void * vars,
			       const char * const * builtin, int nbuiltin)
{
  if (!(nvars >= 0 && (nvars == 0 || (names && vars)))) return { TABLE_INVALID, 0, nullptr };
  for (int q = 0; q < nvars; q++) {
    if (!c_identifier (names[q])) return { TABLE_NO_C_NAME, q, nullptr };
    for (int b = 0; b < nbuiltin; b++)
      if (strcmp (names[q], builtin[b]) == 0) return { TABLE_BUILTIN, q, builtin[b] };
    for (int p = 0; p < q; p++)
      if (strcmp (names[q], names[p]) == 0) return { TABLE_TWICE, q, names[q] };
  }
  return { TABLE_OK, nvars, nullptr };
}

} // namespace gfship
